// The two ends of the reference's optimisation step that are not network layers (train.py:74-89):
//
//   * the deep-supervision loss (train.py:76-85; utils/loss.py:6-11): every output bilinearly resized to the label, then
//     binary_cross_entropy_with_logits + iou_loss, summed over the outputs.  Eagerly that is ~35 framework launches per
//     output over 4.7 MB maps (resize, sigmoid, products, four reductions, their backward); here it is one pass that leaves
//     three sums per image (the resized logit is recomputed from the small map, never stored), one finishing block, and
//     one gradient pass per output that lands directly on the output's own resolution (the resize backward is a gather
//     per source pixel, as in tramba_upsample_bilinear_bwd);
//   * Adam (train.py:266-280, torch.optim.Adam's arithmetic): one read and one write of p / exp_avg / exp_avg_sq and one
//     read of the gradient per step, the tensors of a launch described BY VALUE in the kernel arguments (nothing is
//     copied to the device, hipGraph-capture safe: the gradients of a captured step live at other addresses than the
//     warm-up's);
//   * what sits between backward and Adam when a step is built from several micro-batches (no reference counterpart: the
//     reference steps once per batch): gradient accumulation, the global L2 norm with its clip factor and the "a
//     gradient is not finite: skip this step" decision.  The decisions live in a small record ON THE DEVICE
//     (tramba_step_ctl) that the kernels read and write, so a replayed hipGraph needs no host value that changes from
//     step to step.  Dynamic loss scaling for fp16 activations hangs on the same record: a second one (tramba_loss_scale)
//     holds a power-of-two scale that the loss gradient kernels read through `gscale`, tramba_grad_norm_scaled folds its
//     inverse into the optimizer's scalar, and a one-lane kernel moves it after the optimizer by the record's skip flag;
//
//   * the reference's other two losses (utils/loss.py:14-42: structure_loss, wbce): the same passes with a per-pixel weight
//     map formed once per call from the label (separable box sums in LDS), 12 B per label pixel and output;
//
// All are HBM-streaming kernels: the loss moves 8 B per label pixel and output, Adam 28 B per parameter, an accumulate
// pass 12 B (8 B on the first micro-batch), the norm 4 B.
#include "common.h"

#include <algorithm>
#include <cmath>
#include <type_traits>
#include <vector>

namespace tramba {

// ------------------------------------------------------------------------------------------------- loss
// upsample_bilinear2d (align_corners=False): src = max(scale * (dst + 0.5) - 0.5, 0), i0 = floor(src),
// i1 = i0 + (i0 < n - 1), weights 1 - f, f.
struct Tap {
    int i0, i1;
    float l0, l1;
};
__device__ __forceinline__ Tap tap(int dst, float scale, int n)
{
    const float f = fmaxf(scale * ((float)dst + 0.5f) - 0.5f, 0.f);
    Tap t;
    t.i0 = (int)f;
    t.i1 = t.i0 + (t.i0 < n - 1 ? 1 : 0);
    t.l1 = f - (float)t.i0;
    t.l0 = 1.f - t.l1;
    return t;
}
__device__ __forceinline__ float resized(const float *__restrict__ z, int w, const Tap &ty, const Tap &tx)
{
    const float *r0 = z + (long)ty.i0 * w, *r1 = z + (long)ty.i1 * w;
    return ty.l0 * (tx.l0 * r0[tx.i0] + tx.l1 * r0[tx.i1]) + ty.l1 * (tx.l0 * r1[tx.i0] + tx.l1 * r1[tx.i1]);
}
// sigmoid(z) and log(1 + exp(-|z|)) from one exponential
__device__ __forceinline__ void sig_terms(float z, float &p, float &softplus_tail)
{
    const float e = expf(-fabsf(z)), r = 1.f / (1.f + e);
    p = z >= 0.f ? r : e * r;
    softplus_tail = log1pf(e);
}

constexpr int kLossThreads = 256;

// The per-pixel arithmetic comes in two forms, and every kernel below is written once over them.
//
// PlainLoss: binary_cross_entropy_with_logits + iou_loss (train.py:76-85).  Three sums per block and plane,
//   { sum bce, sum p y, sum (p + y) }, and d loss / d logit = a (p - y) + p (1 - p) (cI y + cU).
// WeightedLoss: structure_loss / wbce (utils/loss.py:14-42), the same passes with a per-pixel weight W = wadd + wmul * wmap[i]
//   -- { 0, 1 } for the box-filter map of loss_weight_map_kernel, { 1, 5 } for a caller's `weight` tensor (utils/loss.py:24)
//   -- and a smoothed BCE target yhat = ysc * y + yadd = (1 - eps) y + eps / 2.  The weight depends on the label only: one map
//   per loss call, shared by the deep-supervision outputs (12 B per label pixel and output instead of 8).  Five sums,
//   { sum bce(z, yhat), sum W bce, sum W, sum W p y, sum W (p + y) } (y unsmoothed in the last two), and
//   d loss / d logit = a omega (p - yhat) + p (1 - p) W (cI y + cU), omega = W in the per-pixel reading of the BCE term, else 1.
// kI: where a row of sums holds I (U follows it).  `i` counts pixels from the start of the tensor.  Each form keeps its own
// expressions: W = 1 through the weighted ones rounds differently from the plain ones.
struct LossCoef {
    float ca, ci, cu;   // gscale * { a, cI, cU } of the plane
    bool pixel;         // omega = W (weighted form only)
};
struct PlainLoss {
    static constexpr int kSums = 3, kI = 1;
    static constexpr bool kWeighted = false;
    __device__ __forceinline__ void add(float (&s)[kSums], long i, float zz, float y, float p, float tail) const
    {
        s[0] += fmaxf(zz, 0.f) - zz * y + tail;
        s[1] = fmaf(p, y, s[1]);
        s[2] += p + y;
    }
    __device__ __forceinline__ float grad(long i, float y, float p, const LossCoef &c) const
    {
        return c.ca * (p - y) + p * (1.f - p) * fmaf(c.ci, y, c.cu);
    }
};
struct WeightedLoss {
    static constexpr int kSums = 5, kI = 3;
    static constexpr bool kWeighted = true;
    const float *wmap;
    float wadd, wmul, ysc, yadd;
    __device__ __forceinline__ void add(float (&s)[kSums], long i, float zz, float y, float p, float tail) const
    {
        const float wt = fmaf(wmul, wmap[i], wadd);
        const float bce = fmaxf(zz, 0.f) - zz * fmaf(ysc, y, yadd) + tail;
        s[0] += bce;
        s[1] = fmaf(wt, bce, s[1]);
        s[2] += wt;
        s[3] = fmaf(wt, p * y, s[3]);
        s[4] = fmaf(wt, p + y, s[4]);
    }
    __device__ __forceinline__ float grad(long i, float y, float p, const LossCoef &c) const
    {
        const float wt = fmaf(wmul, wmap[i], wadd);
        return c.ca * (c.pixel ? wt : 1.f) * (p - fmaf(ysc, y, yadd)) + p * (1.f - p) * wt * fmaf(c.ci, y, c.cu);
    }
};

// part[plane][blockIdx.x][FORM::kSums] = the form's sums over this block's pixels of the plane
template <bool SAME, class FORM>
__global__ __launch_bounds__(kLossThreads) void sod_loss_sums_kernel(const float *__restrict__ z,
                                                                    const float *__restrict__ label,
                                                                    float *__restrict__ part, int h, int w, int H, int W,
                                                                    FORM f)
{
    constexpr int NS = FORM::kSums;
    __shared__ float red[kLossThreads / kWave][NS];
    const int plane = blockIdx.y, nblk = gridDim.x;
    const long npix = (long)H * W;
    const float *zp = z + (long)plane * h * w, *yp = label + plane * npix;
    const float sy = (float)h / (float)H, sx = (float)w / (float)W;
    float s[NS] = {};
    for (long i = (long)blockIdx.x * kLossThreads + threadIdx.x; i < npix; i += (long)nblk * kLossThreads) {
        float zz;
        if constexpr (SAME) {
            zz = zp[i];
        } else {
            const int Y = (int)(i / W), X = (int)(i - (long)Y * W);
            zz = resized(zp, w, tap(Y, sy, h), tap(X, sx, w));
        }
        float p, tail;
        sig_terms(zz, p, tail);
        f.add(s, plane * npix + i, zz, yp[i], p, tail);
    }
    const int lane = threadIdx.x & (kWave - 1), wv = threadIdx.x >> 6;
#pragma unroll
    for (int j = 0; j < NS; ++j) s[j] = wave_sum(s[j]);
    if (lane == 0)
#pragma unroll
        for (int j = 0; j < NS; ++j) red[wv][j] = s[j];
    __syncthreads();
    if (threadIdx.x < NS) {
        float t = 0.f;
        for (int q = 0; q < kLossThreads / kWave; ++q) t += red[q][threadIdx.x];
        part[((long)plane * nblk + blockIdx.x) * NS + threadIdx.x] = t;
    }
}

constexpr int kLossOutputs = 8, kLossPlanes = 512;
struct LossFinishArgs {
    const float *part[kLossOutputs];   // (planes, nblk[i], FORM::kSums)
    float *coef[kLossOutputs];         // (planes, 4): { a, cI, cU, omega selector }
    int nblk[kLossOutputs];
    float weight[kLossOutputs];
    int nout, planes, pixel, iou;      // PlainLoss: pixel = 0, iou = 1
    double npix;
    float *loss;
};
// One block.  Per output o and plane q, with I and U the form's two IoU sums and D = U - I + 1:
//   BCE term, also the reference's weighted losses as they execute (`reduce='none'` resolves to the mean, the weight
//             cancels):                                   sum_q bce_q / (planes npix)
//             per pixel (the weighted losses as published): mean_q (sum W bce)_q / (sum W)_q
//   IoU term (when on): mean_q (1 - (I + 1) / D)
//   loss = sum_o w_o (BCE term + IoU term)
// and the coefficients of d loss / d logit (see the forms above):
//   a = w_o / (planes npix), c[3] = 0;   per pixel: a = w_o / (planes (sum W)_q), c[3] = 1 (omega = W);
//   cI = -(w_o / planes) (U + 2) / D^2,  cU = (w_o / planes) (I + 1) / D^2,  both 0 without the IoU term.
// A wave per (output, plane) adds the partial sums (lanes stride over them, then a shuffle tree: a fixed order).
__device__ __forceinline__ double wave_sum_f64(double v)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}
template <class FORM>
__global__ __launch_bounds__(1024) void sod_loss_finish_kernel(LossFinishArgs a)
{
    constexpr int NS = FORM::kSums;
    __shared__ double term[kLossOutputs][kLossPlanes];
    const int lane = threadIdx.x & (kWave - 1), wv = threadIdx.x >> 6, nwave = blockDim.x >> 6;
    const bool pixel = FORM::kWeighted && a.pixel, iou = !FORM::kWeighted || a.iou;
    for (int item = wv; item < a.nout * a.planes; item += nwave) {
        const int o = item / a.planes, q = item - o * a.planes;
        const float *p = a.part[o] + (long)q * a.nblk[o] * NS;
        double v[NS] = {};
        for (int s = lane; s < a.nblk[o]; s += kWave)
#pragma unroll
            for (int j = 0; j < NS; ++j) v[j] += (double)p[NS * s + j];
#pragma unroll
        for (int j = 0; j < NS; ++j) v[j] = wave_sum_f64(v[j]);
        if (lane == 0) {
            const double w = (double)a.weight[o], planes = (double)a.planes, I = v[FORM::kI], U = v[FORM::kI + 1], D = U - I + 1.0;
            const double bce = pixel ? v[1] / v[2] / planes : v[0] / (planes * a.npix);
            term[o][q] = w * (bce + (iou ? (1.0 - (I + 1.0) / D) / planes : 0.0));
            float *c = a.coef[o] + 4 * (long)q;
            c[0] = (float)(w / (planes * (pixel ? v[2] : a.npix)));
            c[1] = iou ? (float)(-(w / planes) * (U + 2.0) / (D * D)) : 0.f;
            c[2] = iou ? (float)((w / planes) * (I + 1.0) / (D * D)) : 0.f;
            c[3] = pixel ? 1.f : 0.f;
        }
    }
    __syncthreads();
    if (wv == 0) {
        double s = 0.0;
        for (int item = lane; item < a.nout * a.planes; item += kWave) s += term[item / a.planes][item % a.planes];
        s = wave_sum_f64(s);
        if (lane == 0) *a.loss = (float)s;
    }
}

template <class FORM>
__device__ __forceinline__ LossCoef loss_coef(const float *__restrict__ coef, const float *__restrict__ gscale, int plane)
{
    const float gs = gscale ? *gscale : 1.f;
    return {gs * coef[4 * plane], gs * coef[4 * plane + 1], gs * coef[4 * plane + 2],
            FORM::kWeighted && coef[4 * plane + 3] != 0.f};
}
template <class FORM>
__device__ __forceinline__ float loss_grad(const FORM &f, long i, float zz, float y, const LossCoef &c)
{
    float p, tail;
    sig_terms(zz, p, tail);
    return f.grad(i, y, p, c);
}

// same resolution: one thread per pixel
template <class FORM>
__global__ __launch_bounds__(256) void sod_loss_grad_same_kernel(const float *__restrict__ z, const float *__restrict__ label,
                                                                const float *__restrict__ coef,
                                                                const float *__restrict__ gscale, float *__restrict__ gz,
                                                                long npix, FORM f)
{
    const int plane = blockIdx.y;
    const LossCoef c = loss_coef<FORM>(coef, gscale, plane);
    const long base = (long)plane * npix;
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < npix; i += (long)gridDim.x * blockDim.x)
        gz[base + i] = loss_grad(f, base + i, z[base + i], label[base + i], c);
}

// resized output: the adjoint of the bilinear resize is separable, so the gradient at label resolution is formed ONCE per
// label pixel (a row band in LDS) and folded along X, then along Y.  (A gather per source pixel over its 2-D window -- the
// form of tramba_upsample_bilinear_bwd -- evaluates every label pixel ~4 times: 49 us for the 24x24 map of a batch of 8.)
// The label columns / rows that read source index i: a window of (2 / scale + 2) around its centre.
__device__ __forceinline__ void window(int i, float scale, int N, int &lo, int &hi)
{
    lo = max(0, (int)((i - 1 + 0.5f) / scale - 0.5f) - 1);
    hi = min(N - 1, (int)((i + 1 + 0.5f) / scale - 0.5f) + 1);
}
__device__ __forceinline__ float tap_weight(const Tap &t, int i)
{
    return (t.i0 == i ? t.l0 : 0.f) + (t.i1 == i ? t.l1 : 0.f);
}
constexpr int kGradRows = 4;
// rows[plane][Y][x] = sum over X of wx(X -> x) g(Y, X)
template <class FORM>
__global__ __launch_bounds__(256) void sod_loss_grad_rows_kernel(const float *__restrict__ z, const float *__restrict__ label,
                                                                const float *__restrict__ coef,
                                                                const float *__restrict__ gscale, float *__restrict__ rows,
                                                                int h, int w, int H, int W, FORM f)
{
    extern __shared__ float band[];               // [kGradRows][W]
    const int plane = blockIdx.y, yb = blockIdx.x * kGradRows;
    const LossCoef c = loss_coef<FORM>(coef, gscale, plane);
    const float sy = (float)h / (float)H, sx = (float)w / (float)W;
    const long base = (long)plane * H * W;
    const float *zp = z + (long)plane * h * w;
    for (int e = threadIdx.x; e < kGradRows * W; e += blockDim.x) {
        const int r = e / W, X = e - r * W, Y = yb + r;
        const long i = base + (long)Y * W + X;
        if (Y < H) band[e] = loss_grad(f, i, resized(zp, w, tap(Y, sy, h), tap(X, sx, w)), label[i], c);
    }
    __syncthreads();
    for (int e = threadIdx.x; e < kGradRows * w; e += blockDim.x) {
        const int r = e / w, x = e - r * w, Y = yb + r;
        if (Y >= H) continue;
        int X0, X1;
        window(x, sx, W, X0, X1);
        float acc = 0.f;
        for (int X = X0; X <= X1; ++X) acc = fmaf(tap_weight(tap(X, sx, w), x), band[r * W + X], acc);
        rows[((long)plane * H + Y) * w + x] = acc;
    }
}
// gz[plane][y][x] = sum over Y of wy(Y -> y) rows[plane][Y][x]
__global__ __launch_bounds__(256) void sod_loss_grad_cols_kernel(const float *__restrict__ rows, float *__restrict__ gz, int h,
                                                                int w, int H, long total)
{
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= total) return;
    const int x = (int)(i % w);
    const long t = i / w;
    const int y = (int)(t % h);
    const long plane = t / h;
    const float sy = (float)h / (float)H;
    int Y0, Y1;
    window(y, sy, H, Y0, Y1);
    const float *r = rows + plane * (long)H * w + x;
    float acc = 0.f;
    for (int Y = Y0; Y <= Y1; ++Y) acc = fmaf(tap_weight(tap(Y, sy, h), y), r[(long)Y * w], acc);
    gz[i] = acc;
}

// ------------------------------------------------------------------------------------------------- weight map
// weit = 1 + 5 |avg_pool2d(label, k, stride 1, pad k / 2) - label| (utils/loss.py:22, 39), zero padding, divisor k * k
// (count_include_pad): what WeightedLoss reads when the caller gives no weight.  A workgroup owns a 32 x 32 tile: the tile
// with its halo of r = k / 2 goes to LDS (zeros outside the image), row sums of k neighbours into a second LDS band, then
// column sums of those -- every sum in a fixed order that depends on the pixel's position only.
constexpr int kWmapTile = 32, kWmapMaxK = 63;
__global__ __launch_bounds__(256) void loss_weight_map_kernel(const float *__restrict__ label, float *__restrict__ weit, int H,
                                                             int W, int r)
{
    extern __shared__ float wm_lds[];
    const int side = kWmapTile + 2 * r, k = 2 * r + 1;
    float *raw = wm_lds;                    // [side][side]
    float *hs = wm_lds + side * side;       // [side][kWmapTile]
    const int x0 = blockIdx.x * kWmapTile, y0 = blockIdx.y * kWmapTile;
    const long base = (long)blockIdx.z * H * W;
    const float *yp = label + base;
    for (int e = threadIdx.x; e < side * side; e += blockDim.x) {
        const int ry = e / side, rx = e - ry * side, Y = y0 - r + ry, X = x0 - r + rx;
        raw[e] = (Y >= 0 && Y < H && X >= 0 && X < W) ? yp[(long)Y * W + X] : 0.f;
    }
    __syncthreads();
    for (int e = threadIdx.x; e < side * kWmapTile; e += blockDim.x) {
        const float *p = raw + (e / kWmapTile) * side + (e % kWmapTile);
        float s = 0.f;
        for (int d = 0; d < k; ++d) s += p[d];
        hs[e] = s;
    }
    __syncthreads();
    const float kk = (float)(k * k);
    for (int e = threadIdx.x; e < kWmapTile * kWmapTile; e += blockDim.x) {
        const int y = e / kWmapTile, x = e % kWmapTile, Y = y0 + y, X = x0 + x;
        if (Y >= H || X >= W) continue;
        float s = 0.f;
        for (int d = 0; d < k; ++d) s += hs[(y + d) * kWmapTile + x];
        weit[base + (long)Y * W + X] = 1.f + 5.f * fabsf(s / kk - raw[(y + r) * side + x + r]);
    }
}

// ------------------------------------------------------------------------------------------------- Adam
constexpr int kAdamTensors = 72, kAdamSchedTensors = 64, kAdamChunk = 8192, kAdamThreads = 256, kBumpTensors = 448;

// The tensors of one launch, BY VALUE in the kernel arguments: a workgroup per chunk of kAdamChunk elements, tensor after
// tensor.  Every multi-tensor kernel of the optimizer step takes one of these (with its own fields behind it) and finds
// its tensor with tensor_of_block; deal_launches (below, on the host) fills them.
template <class T, int CAP>
struct TensorTable {
    static constexpr int kCap = CAP;
    T t[CAP];                      // (unused slots: zeros)
    int first[CAP + 1];            // first workgroup of each tensor (ascending); first[count..CAP] = the grid
    int count;
};

// the tensor this workgroup works on: first[i] <= blockIdx.x < first[i + 1]
template <typename A>
__device__ __forceinline__ int tensor_of_block(const A &a)
{
    int lo = 0, hi = a.count;
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (a.first[mid] <= (int)blockIdx.x) lo = mid; else hi = mid;
    }
    return lo;
}

struct AdamTensor {
    float *p;
    const float *g;
    float *m, *v;
    const float *step;
    long n;
};
struct AdamSchedTensor : AdamTensor {
    float *e;                      // the average (null: this tensor keeps none)
};
struct AdamHyper {
    double lr, beta1, beta2, eps, weight_decay;
    const float *gscale;           // device scalar the gradient is multiplied by first (null: the gradient as it is)
    const int *skip;               // device flag: non-zero = this launch changes nothing (null: never)
};
// tramba_adam_step / _ctl: 72 tensors of six words.  tramba_adam_step_sched with a record: a seventh pointer per tensor,
// so 64 of them (3912 of the 4096 bytes), and the record the learning-rate factor and the averages' weight live in.
struct AdamArgs : TensorTable<AdamTensor, kAdamTensors> {
    AdamHyper h;
};
struct AdamSchedArgs : TensorTable<AdamSchedTensor, kAdamSchedTensors> {
    AdamHyper h;
    const tramba_step_sched *sched;   // never null (the entry hands a call without one to adam_kernel)
};
struct BumpArgs {
    float *step[kBumpTensors];
    int count;
    const int *skip;
};
static_assert(sizeof(AdamArgs) <= 4096 && sizeof(AdamSchedArgs) <= 4096 && sizeof(BumpArgs) <= 4096,
              "kernel arguments are limited to 4 KB");

__global__ __launch_bounds__(kBumpTensors) void adam_bump_kernel(BumpArgs a)
{
    if (a.skip && *a.skip) return;
    if ((int)threadIdx.x < a.count) *a.step[threadIdx.x] += 1.f;
}

typedef float adam_f4 __attribute__((ext_vector_type(4)));

template <bool ALIGNED>
__device__ __forceinline__ adam_f4 adam_load(const float *p)
{
    if constexpr (ALIGNED) return *reinterpret_cast<const adam_f4 *>(p);
    adam_f4 v = {p[0], p[1], p[2], p[3]};
    return v;
}
template <bool ALIGNED>
__device__ __forceinline__ void adam_store(float *p, adam_f4 v)
{
    if constexpr (ALIGNED) {
        *reinterpret_cast<adam_f4 *>(p) = v;
    } else {
        p[0] = v.x; p[1] = v.y; p[2] = v.z; p[3] = v.w;
    }
}

struct AdamCoef {
    float step_size, bc2_sqrt, b1w, beta2, b2w, eps, wd, gs;
    bool scaled;
};
// torch.optim.Adam (amsgrad off, maximize off):  g += wd p;  m = lerp(m, g, 1 - b1);  v = b2 v + (1 - b2) g g;
// p -= (lr / (1 - b1^t)) m / (sqrt(v) / sqrt(1 - b2^t) + eps)
// A scaled step (tramba_adam_step_ctl) multiplies the gradient first, rounded to fp32 on its own (never contracted into what
// follows): the step equals tramba_adam_step on gradients that were scaled beforehand.
__device__ __forceinline__ void adam_math(float &p, float g, float &m, float &v, const AdamCoef &c)
{
    if (c.scaled) g = __fmul_rn(c.gs, g);
    g = fmaf(c.wd, p, g);
    m = fmaf(c.b1w, g - m, m);
    v = fmaf(c.beta2, v, c.b2w * g * g);
    const float denom = sqrtf(v) / c.bc2_sqrt + c.eps;
    p -= c.step_size * m / denom;
}

// One chunk of one tensor.  EMA: the tensor keeps an average, moved in the same pass by e = fmaf(w, p_new - e, e): one more
// read and write per element (36 B instead of 28).
template <bool ALIGNED, bool EMA>
__device__ __forceinline__ void adam_chunk(const AdamTensor &t, float *avg, long off, const AdamCoef &c, float w)
{
    const long left = t.n - off;
    const int here = left < kAdamChunk ? (int)left : kAdamChunk;
    const int nvec = here >> 2;
    float *p = t.p + off, *m = t.m + off, *v = t.v + off, *e = EMA ? avg + off : nullptr;
    const float *g = t.g + off;
    constexpr int U = 4;
    for (int j0 = threadIdx.x; j0 < nvec; j0 += U * kAdamThreads) {
        adam_f4 pp[U], gg[U], mm[U], vv[U], ee[U];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int j = j0 + u * kAdamThreads;
            if (j < nvec) {
                gg[u] = adam_load<ALIGNED>(g + 4 * j);
                pp[u] = adam_load<ALIGNED>(p + 4 * j);
                mm[u] = adam_load<ALIGNED>(m + 4 * j);
                vv[u] = adam_load<ALIGNED>(v + 4 * j);
                if constexpr (EMA) ee[u] = adam_load<ALIGNED>(e + 4 * j);
            }
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int j = j0 + u * kAdamThreads;
            if (j < nvec) {
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    float pe = pp[u][k], me = mm[u][k], ve = vv[u][k];
                    adam_math(pe, gg[u][k], me, ve, c);
                    pp[u][k] = pe;
                    mm[u][k] = me;
                    vv[u][k] = ve;
                    if constexpr (EMA) ee[u][k] = fmaf(w, pe - ee[u][k], ee[u][k]);
                }
                adam_store<ALIGNED>(p + 4 * j, pp[u]);
                adam_store<ALIGNED>(m + 4 * j, mm[u]);
                adam_store<ALIGNED>(v + 4 * j, vv[u]);
                if constexpr (EMA) adam_store<ALIGNED>(e + 4 * j, ee[u]);
            }
        }
    }
    const int j = (nvec << 2) + threadIdx.x;     // < 4 trailing elements of the tensor
    if (j < here) {
        float pe = p[j], me = m[j], ve = v[j];
        adam_math(pe, g[j], me, ve, c);
        p[j] = pe;
        m[j] = me;
        v[j] = ve;
        if constexpr (EMA) e[j] = fmaf(w, pe - e[j], e[j]);
    }
}

// The one Adam kernel body.  With a schedule record (AdamSchedArgs) the step runs at lr times the record's factor, and a
// tensor that carries an average moves it; without one (AdamArgs) neither is compiled in and no record is read.
template <class ARGS>
__device__ __forceinline__ void adam_body(const ARGS &a)
{
    constexpr bool SCHED = std::is_same<ARGS, AdamSchedArgs>::value;
    __shared__ float corr[2];
    if (a.h.skip && *a.h.skip) return;            // (uniform over the grid: parameters, moments and averages keep their bits)
    const int ti = tensor_of_block(a);
    const auto t = a.t[ti];
    const long off = (long)((int)blockIdx.x - a.first[ti]) * kAdamChunk;
    if (threadIdx.x == 0) {                       // the bias corrections in double, as the reference's optimizer computes them
        const double s = (double)*t.step;
        double lr = a.h.lr;
        if constexpr (SCHED) lr = a.h.lr * a.sched->lr_factor;
        corr[0] = (float)(lr / (1.0 - pow(a.h.beta1, s)));
        corr[1] = (float)sqrt(1.0 - pow(a.h.beta2, s));
    }
    __syncthreads();
    AdamCoef c;
    c.step_size = corr[0];
    c.bc2_sqrt = corr[1];
    c.b1w = (float)(1.0 - a.h.beta1);
    c.beta2 = (float)a.h.beta2;
    c.b2w = (float)(1.0 - a.h.beta2);
    c.eps = (float)a.h.eps;
    c.wd = (float)a.h.weight_decay;
    c.scaled = a.h.gscale != nullptr;
    c.gs = c.scaled ? *a.h.gscale : 1.f;
    uintptr_t bits = reinterpret_cast<uintptr_t>(t.p) | reinterpret_cast<uintptr_t>(t.g) | reinterpret_cast<uintptr_t>(t.m) |
                     reinterpret_cast<uintptr_t>(t.v);
    if constexpr (SCHED) bits |= reinterpret_cast<uintptr_t>(t.e);
    const bool al = (bits & 15) == 0;
    if constexpr (SCHED) {
        if (t.e) {
            const float w = a.sched->ema_weight;
            if (al) adam_chunk<true, true>(t, t.e, off, c, w); else adam_chunk<false, true>(t, t.e, off, c, w);
            return;
        }
    }
    if (al) adam_chunk<true, false>(t, nullptr, off, c, 0.f); else adam_chunk<false, false>(t, nullptr, off, c, 0.f);
}

__global__ __launch_bounds__(kAdamThreads) void adam_kernel(AdamArgs a) { adam_body(a); }
__global__ __launch_bounds__(kAdamThreads) void adam_sched_kernel(AdamSchedArgs a) { adam_body(a); }

// The schedule record's move after a step: one lane, behind the optimizer's launches (and the loss scale's move).  It does
// not read the skip flag: the index counts the steps that were attempted.
__global__ void step_sched_advance_kernel(tramba_step_sched *rec, const double *lr_table, long n_lr, const float *ema_table,
                                          long n_ema)
{
    if (blockIdx.x != 0 || threadIdx.x != 0) return;
    const long step = (long)rec->step + 1;
    const long at = step < 0 ? 0 : step;          // (a record filled with a negative count reads the first entries)
    rec->step = step;
    rec->lr_factor = lr_table ? lr_table[at < n_lr - 1 ? at : n_lr - 1] : 1.0;
    if (ema_table) rec->ema_weight = ema_table[at < n_ema - 1 ? at : n_ema - 1];
}

// ------------------------------------------------------------------------------------------------- step control
// Tensors of a launch are dealt like Adam's: by value in the kernel arguments, a workgroup per chunk of kAdamChunk elements.
constexpr int kAccTensors = 128, kNormTensors = 160, kNormThreads = 256;
struct AccTensor {
    float *acc;
    const float *g;                // null: this micro-batch produced no gradient for the tensor (zeros)
    long n;
};
struct AccArgs : TensorTable<AccTensor, kAccTensors> {
    const tramba_step_ctl *ctl;
};
struct NormTensor {
    const float *g;
    long n;
};
struct NormArgs : TensorTable<NormTensor, kNormTensors> {
    int chunk_base;                // this launch's first slot in the tables of partials
    double *part;
    unsigned *bad;
};
static_assert(sizeof(AccArgs) <= 4096 && sizeof(NormArgs) <= 4096, "kernel arguments are limited to 4 KB");

// acc = g on the first micro-batch of a step (ctl->micro == 0), acc += g afterwards
template <bool ALIGNED>
__device__ __forceinline__ void acc_chunk(float *acc, const float *g, int here, bool first)
{
    const int nvec = here >> 2;
    constexpr int U = 4;
    for (int j0 = threadIdx.x; j0 < nvec; j0 += U * kAdamThreads) {
        adam_f4 aa[U], gg[U];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int j = j0 + u * kAdamThreads;
            if (j < nvec) {
                gg[u] = g ? adam_load<ALIGNED>(g + 4 * j) : adam_f4{0.f, 0.f, 0.f, 0.f};
                if (!first) aa[u] = adam_load<ALIGNED>(acc + 4 * j);
            }
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int j = j0 + u * kAdamThreads;
            if (j < nvec) adam_store<ALIGNED>(acc + 4 * j, first ? gg[u] : aa[u] + gg[u]);
        }
    }
    const int j = (nvec << 2) + threadIdx.x;
    if (j < here) {
        const float ge = g ? g[j] : 0.f;
        acc[j] = first ? ge : acc[j] + ge;
    }
}

__global__ __launch_bounds__(kAdamThreads) void grad_accumulate_kernel(AccArgs a)
{
    const int ti = tensor_of_block(a);
    const AccTensor t = a.t[ti];
    const bool first = a.ctl->micro == 0;
    if (!t.g && !first) return;                   // nothing to add
    const long off = (long)((int)blockIdx.x - a.first[ti]) * kAdamChunk;
    const long left = t.n - off;
    const int here = left < kAdamChunk ? (int)left : kAdamChunk;
    const float *g = t.g ? t.g + off : nullptr;
    const bool al = ((reinterpret_cast<uintptr_t>(t.acc) | reinterpret_cast<uintptr_t>(t.g)) & 15) == 0;
    if (al) acc_chunk<true>(t.acc + off, g, here, first); else acc_chunk<false>(t.acc + off, g, here, first);
}

__global__ void step_ctl_advance_kernel(tramba_step_ctl *ctl)
{
    if (threadIdx.x == 0) ctl->micro += 1;
}

// part[chunk] = sum of squares of the chunk in fp64 (products of fp32 values are exact there), bad[chunk] = any element
// with an all-ones exponent (Inf / NaN): decided per element, a sum can overflow or cancel its way to either verdict
__global__ __launch_bounds__(kNormThreads) void grad_norm_parts_kernel(NormArgs a)
{
    __shared__ double red[kNormThreads / kWave];
    __shared__ unsigned redbad[kNormThreads / kWave];
    const int ti = tensor_of_block(a);
    const NormTensor t = a.t[ti];
    const long off = (long)((int)blockIdx.x - a.first[ti]) * kAdamChunk;
    const long left = t.n - off;
    const int here = left < kAdamChunk ? (int)left : kAdamChunk;
    const float *g = t.g + off;
    double s = 0.0;
    unsigned bad = 0;
    auto take = [&](float x) {
        bad |= (__float_as_uint(x) & 0x7f800000u) == 0x7f800000u;
        s = fma((double)x, (double)x, s);
    };
    if ((reinterpret_cast<uintptr_t>(g) & 15) == 0) {
        const int nvec = here >> 2;
        constexpr int U = 4;
        for (int j0 = threadIdx.x; j0 < nvec; j0 += U * kNormThreads) {
            adam_f4 gg[U];
#pragma unroll
            for (int u = 0; u < U; ++u) {
                const int j = j0 + u * kNormThreads;
                gg[u] = j < nvec ? adam_load<true>(g + 4 * j) : adam_f4{0.f, 0.f, 0.f, 0.f};
            }
#pragma unroll
            for (int u = 0; u < U; ++u)
#pragma unroll
                for (int e = 0; e < 4; ++e) take(gg[u][e]);
        }
        const int j = (nvec << 2) + threadIdx.x;
        if (j < here) take(g[j]);
    } else {
        for (int j = threadIdx.x; j < here; j += kNormThreads) take(g[j]);
    }
    s = wave_sum_f64(s);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) bad |= __shfl_xor(bad, o, 64);
    const int lane = threadIdx.x & (kWave - 1), wv = threadIdx.x >> 6;
    if (lane == 0) {
        red[wv] = s;
        redbad[wv] = bad;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        double tot = 0.0;
        unsigned b = 0;
        for (int q = 0; q < kNormThreads / kWave; ++q) {
            tot += red[q];
            b |= redbad[q];
        }
        a.part[a.chunk_base + blockIdx.x] = tot;
        a.bad[a.chunk_base + blockIdx.x] = b;
    }
}

// One block adds the partials in a fixed order (a thread strides over the chunks, a shuffle tree per wave, the waves in
// order) and writes the record.
constexpr int kNormFinishThreads = 1024;
__global__ __launch_bounds__(kNormFinishThreads) void grad_norm_finish_kernel(const double *__restrict__ part,
                                                                             const unsigned *__restrict__ bad, int nchunk,
                                                                             double mean_scale, double max_norm,
                                                                             int skip_nonfinite, tramba_step_ctl *ctl,
                                                                             const tramba_loss_scale *ls)
{
    __shared__ double red[kNormFinishThreads / kWave];
    __shared__ unsigned redbad[kNormFinishThreads / kWave];
    double s = 0.0;
    unsigned b = 0;
    for (int i = threadIdx.x; i < nchunk; i += kNormFinishThreads) {
        s += part[i];
        b |= bad[i];
    }
    s = wave_sum_f64(s);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) b |= __shfl_xor(b, o, 64);
    const int lane = threadIdx.x & (kWave - 1), wv = threadIdx.x >> 6;
    if (lane == 0) {
        red[wv] = s;
        redbad[wv] = b;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        double tot = 0.0;
        unsigned any = 0;
        for (int q = 0; q < kNormFinishThreads / kWave; ++q) {
            tot += red[q];
            any |= redbad[q];
        }
        // gradients that carry a loss scale 2^k: the mean and the un-scaling are one exact factor (ls null: mean_scale as given)
        if (ls) mean_scale *= (double)ls->inv_scale;
        const float norm = (float)(sqrt(tot) * mean_scale);
        double scale = mean_scale;
        if (max_norm > 0.0) {                       // torch.nn.utils.clip_grad_norm_: min(1, max_norm / (norm + 1e-6))
            const double coef = max_norm / ((double)norm + 1e-6);
            scale = mean_scale * (coef < 1.0 ? coef : 1.0);   // (a NaN norm gives a NaN scale, as torch's clamp does)
            if (coef != coef) scale = coef;
        }
        const int skip = (any && skip_nonfinite) ? 1 : 0;
        ctl->norm = norm;
        ctl->scale = (float)scale;
        ctl->skip = skip;
        ctl->micro = 0;
        ctl->skipped_steps += skip;
    }
}

// The loss scale's move after a step: one lane.  Every quantity is a power of two inside fp32's normal range (the entry
// checks the hyper-parameters, the clamps keep the scale there), so products and the division are exact.
__global__ void loss_scale_update_kernel(tramba_loss_scale *ls, const tramba_step_ctl *ctl, float growth, float backoff,
                                         int growth_interval, float min_scale, float max_scale)
{
    if (blockIdx.x != 0 || threadIdx.x != 0) return;
    float scale = ls->scale;
    int good = ls->good_steps;
    if (ctl->skip != 0) {
        scale = fmaxf(min_scale, scale * backoff);
        good = 0;
        ls->backoffs += 1;
    } else if (++good >= growth_interval) {
        scale = fminf(max_scale, scale * growth);
        good = 0;
    }
    ls->scale = scale;
    ls->inv_scale = __fdiv_rn(1.0f, scale);
    ls->good_steps = good;
}

// the tensors dealt to ceil(count / per_launch) launches of equal weight: largest first, in snake order
static std::vector<std::vector<int>> snake_bins(const int64_t *numel, int count, int per_launch)
{
    const int nlaunch = (count + per_launch - 1) / per_launch;
    std::vector<int> order(count);
    for (int i = 0; i < count; ++i) order[i] = i;
    std::stable_sort(order.begin(), order.end(), [&](int x, int y) { return numel[x] > numel[y]; });
    std::vector<std::vector<int>> bins(nlaunch);
    for (int i = 0; i < count; ++i) {
        const int round = i / nlaunch, pos = i % nlaunch;
        bins[(round & 1) ? nlaunch - 1 - pos : pos].push_back(order[i]);
    }
    return bins;
}

// chunks (= workgroups) over all tensors of a call, -1 beyond what a grid holds
static long norm_chunks(const int64_t *numel, int count)
{
    long n = 0;
    for (int i = 0; i < count; ++i) {
        if (numel[i] <= 0) return -1;
        n += (numel[i] + kAdamChunk - 1) / kAdamChunk;
        if (n >= 2147483647L) return -1;
    }
    return n;
}

// The launches of one call over `count` tensors of numel[] elements: the tensors are dealt to ceil(count / ARGS::kCap)
// launches (a launch of 72 bias vectors alone would put 72 workgroups on 256 CUs; the order does not matter, the tensors
// are independent), make(j) is the record of tensor j, launch(table, workgroups) fills in the kernel's own fields and
// starts it.  A call that would not fit a grid is refused before its first launch.
template <class ARGS, class MAKE, class LAUNCH>
static int deal_launches(const char *who, const int64_t *numel, int count, MAKE make, LAUNCH launch)
{
    TRAMBA_CHECK(norm_chunks(numel, count) > 0, "%s: too many workgroups", who);
    for (const std::vector<int> &bin : snake_bins(numel, count, ARGS::kCap)) {
        ARGS a;
        long blocks = 0;
        const int c = (int)bin.size();             // <= kCap by construction
        for (int i = 0; i < c; ++i) {
            a.t[i] = make(bin[i]);
            a.first[i] = (int)blocks;
            blocks += (numel[bin[i]] + kAdamChunk - 1) / kAdamChunk;
        }
        for (int i = c; i < ARGS::kCap; ++i) a.t[i] = {};
        for (int i = c; i <= ARGS::kCap; ++i) a.first[i] = (int)blocks;
        a.count = c;
        if (const int e = launch(a, (unsigned)blocks)) return e;
    }
    return TRAMBA_OK;
}

}  // namespace tramba

using namespace tramba;

// The loss entries come in pairs, tramba_sod_loss_* and tramba_sod_wloss_*: each pair is two wrappers that name themselves
// (`who`, for the error texts) and pick the form over one implementation.
template <class FORM>
static int launch_loss_sums(const char *who, const FORM &f, const float *logits, const float *label, float *part, int planes, int h,
                     int w, int hout, int wout, int nblk, void *stream)
{
    TRAMBA_CHECK(logits && label && part, "%s: null tensor", who);
    TRAMBA_CHECK(planes > 0 && planes <= 65535 && h > 0 && w > 0 && hout > 0 && wout > 0 && nblk > 0, "%s: bad shape", who);
    const dim3 grid((unsigned)nblk, (unsigned)planes);
    if (h == hout && w == wout)
        hipLaunchKernelGGL((sod_loss_sums_kernel<true, FORM>), grid, dim3(kLossThreads), 0, (hipStream_t)stream, logits, label,
                           part, h, w, hout, wout, f);
    else
        hipLaunchKernelGGL((sod_loss_sums_kernel<false, FORM>), grid, dim3(kLossThreads), 0, (hipStream_t)stream, logits, label,
                           part, h, w, hout, wout, f);
    TRAMBA_LAUNCH_CHECK();
    return TRAMBA_OK;
}

static int launch_loss_finish(const char *who, bool weighted, const float *const *parts, const int *nblk, const float *weights,
                       float *const *coefs, int nout, int planes, int64_t npix, int per_pixel, int with_iou, float *loss,
                       void *stream)
{
    TRAMBA_CHECK(parts && nblk && coefs && loss, "%s: null argument", who);
    TRAMBA_CHECK(nout > 0 && nout <= kLossOutputs, "%s: 1..%d outputs (got %d)", who, kLossOutputs, nout);
    TRAMBA_CHECK(planes > 0 && planes <= kLossPlanes && npix > 0, "%s: 1..%d planes (got %d)", who, kLossPlanes, planes);
    LossFinishArgs a;
    for (int o = 0; o < kLossOutputs; ++o) {
        const bool on = o < nout;
        TRAMBA_CHECK(!on || (parts[o] && coefs[o] && nblk[o] > 0), "%s: output %d: null table", who, o);
        a.part[o] = on ? parts[o] : nullptr;
        a.coef[o] = on ? coefs[o] : nullptr;
        a.nblk[o] = on ? nblk[o] : 0;
        a.weight[o] = on ? (weights ? weights[o] : 1.f) : 0.f;
    }
    a.nout = nout;
    a.planes = planes;
    a.pixel = per_pixel != 0;
    a.iou = with_iou != 0;
    a.npix = (double)npix;
    a.loss = loss;
    if (weighted)
        hipLaunchKernelGGL(sod_loss_finish_kernel<WeightedLoss>, dim3(1), dim3(1024), 0, (hipStream_t)stream, a);
    else
        hipLaunchKernelGGL(sod_loss_finish_kernel<PlainLoss>, dim3(1), dim3(1024), 0, (hipStream_t)stream, a);
    TRAMBA_LAUNCH_CHECK();
    return TRAMBA_OK;
}

extern "C" size_t tramba_sod_loss_grad_workspace(int planes, int h, int w, int hout, int wout)
{
    return (h == hout && w == wout) ? 0 : (size_t)planes * (size_t)hout * (size_t)w * sizeof(float);
}

template <class FORM>
static int launch_loss_grad(const char *who, const FORM &f, const float *logits, const float *label, const float *coef,
                     const float *gscale, float *glogits, void *workspace, size_t workspace_bytes, int planes, int h, int w,
                     int hout, int wout, void *stream)
{
    TRAMBA_CHECK(logits && label && coef && glogits, "%s: null tensor", who);
    TRAMBA_CHECK(planes > 0 && planes <= 65535 && h > 0 && w > 0, "%s: bad shape", who);
    hipStream_t s = (hipStream_t)stream;
    if (h == hout && w == wout) {
        const long npix = (long)h * w;
        const unsigned gx = (unsigned)((npix + 1023) / 1024);
        hipLaunchKernelGGL(sod_loss_grad_same_kernel<FORM>, dim3(gx, (unsigned)planes), dim3(256), 0, s, logits, label, coef,
                           gscale, glogits, npix, f);
    } else {
        TRAMBA_CHECK(hout >= h && wout >= w, "%s: outputs are resized UP to the label (%dx%d -> %dx%d)", who, h, w, hout, wout);
        TRAMBA_CHECK(wout <= 4096, "%s: label rows of at most 4096 pixels (got %d)", who, wout);
        TRAMBA_CHECK(workspace && workspace_bytes >= tramba_sod_loss_grad_workspace(planes, h, w, hout, wout),
                     "%s: workspace of %zu bytes needed", who, tramba_sod_loss_grad_workspace(planes, h, w, hout, wout));
        float *rows = (float *)workspace;
        hipLaunchKernelGGL(sod_loss_grad_rows_kernel<FORM>, dim3((unsigned)((hout + kGradRows - 1) / kGradRows), (unsigned)planes),
                           dim3(256), (size_t)kGradRows * wout * sizeof(float), s, logits, label, coef, gscale, rows, h, w, hout,
                           wout, f);
        TRAMBA_LAUNCH_CHECK();
        const long total = (long)planes * h * w;
        TRAMBA_CHECK((total + 255) / 256 < 2147483647L, "%s: too many workgroups", who);
        hipLaunchKernelGGL(sod_loss_grad_cols_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, rows, glogits, h, w,
                           hout, total);
    }
    TRAMBA_LAUNCH_CHECK();
    return TRAMBA_OK;
}

extern "C" int tramba_sod_loss_sums(const float *logits, const float *label, float *part, int planes, int h, int w,
                                    int hout, int wout, int nblk, void *stream)
{
    return launch_loss_sums("sod_loss_sums", PlainLoss{}, logits, label, part, planes, h, w, hout, wout, nblk, stream);
}

extern "C" int tramba_sod_loss_finish(const float *const *parts, const int *nblk, const float *weights, float *const *coefs,
                                      int nout, int planes, int64_t npix, float *loss, void *stream)
{
    return launch_loss_finish("sod_loss_finish", false, parts, nblk, weights, coefs, nout, planes, npix, 0, 1, loss, stream);
}

extern "C" int tramba_sod_loss_grad(const float *logits, const float *label, const float *coef, const float *gscale,
                                    float *glogits, void *workspace, size_t workspace_bytes, int planes, int h, int w,
                                    int hout, int wout, void *stream)
{
    return launch_loss_grad("sod_loss_grad", PlainLoss{}, logits, label, coef, gscale, glogits, workspace, workspace_bytes, planes, h, w,
                     hout, wout, stream);
}

extern "C" int tramba_loss_weight_map(const float *label, float *weit, int planes, int h, int w, int k, void *stream)
{
    TRAMBA_CHECK(label && weit, "loss_weight_map: null tensor");
    TRAMBA_CHECK(planes > 0 && planes <= 65535 && h > 0 && w > 0, "loss_weight_map: bad shape");
    TRAMBA_CHECK(k >= 1 && k <= kWmapMaxK && (k & 1), "loss_weight_map: odd windows of 1..%d (got %d)", kWmapMaxK, k);
    const long gx = ((long)w + kWmapTile - 1) / kWmapTile, gy = ((long)h + kWmapTile - 1) / kWmapTile;
    TRAMBA_CHECK(gy <= 65535, "loss_weight_map: at most %d rows (got %d)", 65535 * kWmapTile, h);
    const int r = k / 2, side = kWmapTile + 2 * r;
    hipLaunchKernelGGL(loss_weight_map_kernel, dim3((unsigned)gx, (unsigned)gy, (unsigned)planes), dim3(256),
                       (size_t)(side * side + side * kWmapTile) * sizeof(float), (hipStream_t)stream, label, weit, h, w, r);
    TRAMBA_LAUNCH_CHECK();
    return TRAMBA_OK;
}

// the form the two weighted entries that read the map are called with
static int weighted_form(const char *who, const float *wmap, float eps, int weight_is_raw, WeightedLoss &f)
{
    TRAMBA_CHECK(wmap, "%s: null tensor", who);
    TRAMBA_CHECK(eps >= 0.f && eps < 1.f, "%s: label smoothing in [0, 1)", who);
    f = weight_is_raw ? WeightedLoss{wmap, 1.f, 5.f, 1.f - eps, 0.5f * eps} : WeightedLoss{wmap, 0.f, 1.f, 1.f - eps, 0.5f * eps};
    return TRAMBA_OK;
}

extern "C" int tramba_sod_wloss_sums(const float *logits, const float *label, const float *wmap, float *part, int planes,
                                     int h, int w, int hout, int wout, int nblk, float eps, int weight_is_raw, void *stream)
{
    WeightedLoss f;
    if (const int e = weighted_form("sod_wloss_sums", wmap, eps, weight_is_raw, f)) return e;
    return launch_loss_sums("sod_wloss_sums", f, logits, label, part, planes, h, w, hout, wout, nblk, stream);
}

extern "C" int tramba_sod_wloss_finish(const float *const *parts, const int *nblk, const float *weights, float *const *coefs,
                                       int nout, int planes, int64_t npix, int per_pixel, int with_iou, float *loss,
                                       void *stream)
{
    return launch_loss_finish("sod_wloss_finish", true, parts, nblk, weights, coefs, nout, planes, npix, per_pixel, with_iou, loss,
                       stream);
}

extern "C" size_t tramba_sod_wloss_grad_workspace(int planes, int h, int w, int hout, int wout)
{
    return tramba_sod_loss_grad_workspace(planes, h, w, hout, wout);
}

extern "C" int tramba_sod_wloss_grad(const float *logits, const float *label, const float *wmap, const float *coef,
                                     const float *gscale, float *glogits, void *workspace, size_t workspace_bytes, int planes,
                                     int h, int w, int hout, int wout, float eps, int weight_is_raw, void *stream)
{
    WeightedLoss f;
    if (const int e = weighted_form("sod_wloss_grad", wmap, eps, weight_is_raw, f)) return e;
    return launch_loss_grad("sod_wloss_grad", f, logits, label, coef, gscale, glogits, workspace, workspace_bytes, planes, h, w, hout,
                     wout, stream);
}

// The one Adam entry behind tramba_adam_step (gscale, skip, ema, sched null), tramba_adam_step_ctl (ema, sched null) and
// tramba_adam_step_sched; `who` names the entry in the error texts.  sched null: adam_kernel, which reads no record.
static int adam_step_impl(const char *who, float *const *params, const float *const *grads, float *const *exp_avg,
                          float *const *exp_avg_sq, float *const *steps, const int64_t *numel, int count, double lr, double beta1,
                          double beta2, double eps, double weight_decay, const float *gscale, const int *skip, float *const *ema,
                          const tramba_step_sched *sched, void *stream)
{
    TRAMBA_CHECK(params && grads && exp_avg && exp_avg_sq && steps && numel && count > 0, "%s: empty input", who);
    TRAMBA_CHECK(lr >= 0.0 && beta1 >= 0.0 && beta1 < 1.0 && beta2 >= 0.0 && beta2 < 1.0 && eps >= 0.0 && weight_decay >= 0.0,
                 "%s: bad hyper-parameters", who);
    hipStream_t s = (hipStream_t)stream;
    for (int i = 0; i < count; ++i) {
        TRAMBA_CHECK(params[i] && grads[i] && exp_avg[i] && exp_avg_sq[i] && steps[i] && numel[i] > 0,
                     "%s: tensor %d: null pointer or no elements", who, i);
        TRAMBA_CHECK(!ema || ema[i], "%s: tensor %d: null average", who, i);
    }
    TRAMBA_CHECK(norm_chunks(numel, count) > 0, "%s: too many workgroups", who);   // (before the counters move)
    for (int base = 0; base < count; base += kBumpTensors) {     // t += 1 on the device (the counters are part of the state_dict)
        BumpArgs b;
        b.count = count - base < kBumpTensors ? count - base : kBumpTensors;
        for (int i = 0; i < kBumpTensors; ++i) b.step[i] = i < b.count ? steps[base + i] : nullptr;
        b.skip = skip;
        hipLaunchKernelGGL(adam_bump_kernel, dim3(1), dim3(kBumpTensors), 0, s, b);
        TRAMBA_LAUNCH_CHECK();
    }
    const AdamHyper h{lr, beta1, beta2, eps, weight_decay, gscale, skip};
    auto tensor = [&](int j) { return AdamTensor{params[j], grads[j], exp_avg[j], exp_avg_sq[j], steps[j], (long)numel[j]}; };
    if (!sched)
        return deal_launches<AdamArgs>(who, numel, count, tensor, [&](AdamArgs &a, unsigned blocks) -> int {
            a.h = h;
            hipLaunchKernelGGL(adam_kernel, dim3(blocks), dim3(kAdamThreads), 0, s, a);
            TRAMBA_LAUNCH_CHECK();
            return TRAMBA_OK;
        });
    return deal_launches<AdamSchedArgs>(
        who, numel, count, [&](int j) { return AdamSchedTensor{tensor(j), ema ? ema[j] : nullptr}; },
        [&](AdamSchedArgs &a, unsigned blocks) -> int {
            a.h = h;
            a.sched = sched;
            hipLaunchKernelGGL(adam_sched_kernel, dim3(blocks), dim3(kAdamThreads), 0, s, a);
            TRAMBA_LAUNCH_CHECK();
            return TRAMBA_OK;
        });
}

extern "C" int tramba_adam_step(float *const *params, const float *const *grads, float *const *exp_avg,
                                float *const *exp_avg_sq, float *const *steps, const int64_t *numel, int count, double lr,
                                double beta1, double beta2, double eps, double weight_decay, void *stream)
{
    return adam_step_impl("adam_step", params, grads, exp_avg, exp_avg_sq, steps, numel, count, lr, beta1, beta2, eps, weight_decay,
                          nullptr, nullptr, nullptr, nullptr, stream);
}

extern "C" int tramba_adam_step_ctl(float *const *params, const float *const *grads, float *const *exp_avg,
                                    float *const *exp_avg_sq, float *const *steps, const int64_t *numel, int count, double lr,
                                    double beta1, double beta2, double eps, double weight_decay, const float *gscale,
                                    const int *skip, void *stream)
{
    return adam_step_impl("adam_step_ctl", params, grads, exp_avg, exp_avg_sq, steps, numel, count, lr, beta1, beta2, eps,
                          weight_decay, gscale, skip, nullptr, nullptr, stream);
}

extern "C" int tramba_adam_step_sched(float *const *params, const float *const *grads, float *const *exp_avg,
                                      float *const *exp_avg_sq, float *const *steps, const int64_t *numel, int count, double lr,
                                      double beta1, double beta2, double eps, double weight_decay, const float *gscale,
                                      const int *skip, float *const *ema, const tramba_step_sched *sched, void *stream)
{
    TRAMBA_CHECK(sched || !ema, "adam_step_sched: an average needs the schedule record (its weight lives there)");
    return adam_step_impl("adam_step_sched", params, grads, exp_avg, exp_avg_sq, steps, numel, count, lr, beta1, beta2, eps,
                          weight_decay, gscale, skip, ema, sched, stream);
}

extern "C" int tramba_step_sched_advance(tramba_step_sched *rec, const double *lr_table, int64_t n_lr, const float *ema_table,
                                         int64_t n_ema, void *stream)
{
    TRAMBA_CHECK(rec, "step_sched_advance: null record");
    TRAMBA_CHECK(!lr_table || n_lr >= 1, "step_sched_advance: an lr table of %lld entries (at least 1)", (long long)n_lr);
    TRAMBA_CHECK(!ema_table || n_ema >= 1, "step_sched_advance: an ema table of %lld entries (at least 1)", (long long)n_ema);
    hipLaunchKernelGGL(step_sched_advance_kernel, dim3(1), dim3(kWave), 0, (hipStream_t)stream, rec, lr_table, (long)n_lr,
                       ema_table, (long)n_ema);
    TRAMBA_LAUNCH_CHECK();
    return TRAMBA_OK;
}

extern "C" int tramba_grad_accumulate(float *const *acc, const float *const *grads, const int64_t *numel, int count,
                                      tramba_step_ctl *ctl, void *stream)
{
    TRAMBA_CHECK(acc && grads && numel && ctl, "grad_accumulate: null argument");
    TRAMBA_CHECK(count > 0, "grad_accumulate: count must be positive (got %d)", count);
    for (int i = 0; i < count; ++i)
        TRAMBA_CHECK(acc[i] && numel[i] > 0, "grad_accumulate: tensor %d: null accumulator or no elements", i);
    hipStream_t s = (hipStream_t)stream;
    const int e = deal_launches<AccArgs>(
        "grad_accumulate", numel, count, [&](int j) { return AccTensor{acc[j], grads[j], (long)numel[j]}; },
        [&](AccArgs &a, unsigned blocks) -> int {
            a.ctl = ctl;
            hipLaunchKernelGGL(grad_accumulate_kernel, dim3(blocks), dim3(kAdamThreads), 0, s, a);
            TRAMBA_LAUNCH_CHECK();
            return TRAMBA_OK;
        });
    if (e) return e;
    hipLaunchKernelGGL(step_ctl_advance_kernel, dim3(1), dim3(kWave), 0, s, ctl);   // after every read of the counter
    TRAMBA_LAUNCH_CHECK();
    return TRAMBA_OK;
}

extern "C" size_t tramba_grad_norm_workspace(const int64_t *numel, int count)
{
    if (!numel || count <= 0) return 0;
    const long n = norm_chunks(numel, count);
    return n < 0 ? 0 : (size_t)n * (sizeof(double) + sizeof(unsigned));
}

static int grad_norm_impl(const float *const *grads, const int64_t *numel, int count, double mean_scale, double max_norm,
                          int skip_nonfinite, tramba_step_ctl *ctl, const tramba_loss_scale *ls, void *workspace,
                          size_t workspace_bytes, void *stream)
{
    TRAMBA_CHECK(grads && numel && ctl && workspace, "grad_norm: null argument");
    TRAMBA_CHECK(count > 0, "grad_norm: count must be positive (got %d)", count);
    TRAMBA_CHECK(mean_scale > 0.0, "grad_norm: mean_scale must be positive");
    for (int i = 0; i < count; ++i)
        TRAMBA_CHECK(grads[i] && numel[i] > 0, "grad_norm: tensor %d: null pointer or no elements", i);
    const long nchunk = norm_chunks(numel, count);
    TRAMBA_CHECK(nchunk > 0, "grad_norm: too many workgroups");   // (here: the workspace's layout follows from the count)
    TRAMBA_CHECK(workspace_bytes >= tramba_grad_norm_workspace(numel, count) && (reinterpret_cast<uintptr_t>(workspace) & 7) == 0,
                 "grad_norm: an 8-byte aligned workspace of %zu bytes needed", tramba_grad_norm_workspace(numel, count));
    hipStream_t s = (hipStream_t)stream;
    double *part = (double *)workspace;
    unsigned *bad = (unsigned *)(part + nchunk);
    long base = 0;
    const int e = deal_launches<NormArgs>(
        "grad_norm", numel, count, [&](int j) { return NormTensor{grads[j], (long)numel[j]}; },
        [&](NormArgs &a, unsigned blocks) -> int {
            a.chunk_base = (int)base;
            a.part = part;
            a.bad = bad;
            hipLaunchKernelGGL(grad_norm_parts_kernel, dim3(blocks), dim3(kNormThreads), 0, s, a);
            TRAMBA_LAUNCH_CHECK();
            base += blocks;
            return TRAMBA_OK;
        });
    if (e) return e;
    hipLaunchKernelGGL(grad_norm_finish_kernel, dim3(1), dim3(kNormFinishThreads), 0, s, part, bad, (int)nchunk, mean_scale,
                       max_norm, skip_nonfinite, ctl, ls);
    TRAMBA_LAUNCH_CHECK();
    return TRAMBA_OK;
}

extern "C" int tramba_grad_norm(const float *const *grads, const int64_t *numel, int count, double mean_scale, double max_norm,
                                int skip_nonfinite, tramba_step_ctl *ctl, void *workspace, size_t workspace_bytes, void *stream)
{
    return grad_norm_impl(grads, numel, count, mean_scale, max_norm, skip_nonfinite, ctl, nullptr, workspace, workspace_bytes,
                          stream);
}

extern "C" int tramba_grad_norm_scaled(const float *const *grads, const int64_t *numel, int count, double mean_scale,
                                       double max_norm, int skip_nonfinite, tramba_step_ctl *ctl, const tramba_loss_scale *ls,
                                       void *workspace, size_t workspace_bytes, void *stream)
{
    return grad_norm_impl(grads, numel, count, mean_scale, max_norm, skip_nonfinite, ctl, ls, workspace, workspace_bytes, stream);
}

// 2^k with 2^k and 2^-k both normal in fp32
static bool pow2_f32(double x)
{
    int e = 0;
    return x > 0.0 && std::frexp(x, &e) == 0.5 && e - 1 >= -126 && e - 1 <= 126;
}

extern "C" int tramba_loss_scale_update(tramba_loss_scale *ls, const tramba_step_ctl *ctl, double growth, double backoff,
                                        int growth_interval, double min_scale, double max_scale, void *stream)
{
    TRAMBA_CHECK(ls && ctl, "loss_scale_update: null argument");
    TRAMBA_CHECK(pow2_f32(growth) && growth > 1.0, "loss_scale_update: growth must be a power of two above 1 (got %g)", growth);
    TRAMBA_CHECK(pow2_f32(backoff) && backoff < 1.0, "loss_scale_update: backoff must be a power of two below 1 (got %g)", backoff);
    TRAMBA_CHECK(growth_interval >= 1, "loss_scale_update: growth_interval must be at least 1 (got %d)", growth_interval);
    TRAMBA_CHECK(pow2_f32(min_scale), "loss_scale_update: min_scale must be a power of two in 2^-126 .. 2^126 (got %g)", min_scale);
    TRAMBA_CHECK(pow2_f32(max_scale), "loss_scale_update: max_scale must be a power of two in 2^-126 .. 2^126 (got %g)", max_scale);
    TRAMBA_CHECK(min_scale <= max_scale, "loss_scale_update: min_scale %g above max_scale %g", min_scale, max_scale);
    hipLaunchKernelGGL(loss_scale_update_kernel, dim3(1), dim3(kWave), 0, (hipStream_t)stream, ls, ctl, (float)growth,
                       (float)backoff, growth_interval, (float)min_scale, (float)max_scale);
    TRAMBA_LAUNCH_CHECK();
    return TRAMBA_OK;
}
