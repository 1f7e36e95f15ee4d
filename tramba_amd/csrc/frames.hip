// The two ends of the deployment pipeline on the device: camera frames in, full-size saliency maps out.
//
// frames_to_input_kernel: (B, H, W, 3) u8 frames -> (B, 3, S, S) f32 model input, bit for bit what the loader's test
//   transform gives (data.get_transform(S, "Test"): PIL Image.resize(BILINEAR) then to_tensors).  The resize is Pillow's
//   separable 8-bit bilinear resample: a horizontal pass into a u8 intermediate, then a vertical pass, each
//   acc = 2^21 + sum px_j k_j with fixed-point weights k_j (22 fractional bits), written as clamp(acc >> 22, 0, 255).  The
//   weights come from tramba_resize_table (host, fp64, FP contraction off), which also holds the 3 x 256 normalisation
//   table (f / 255 in fp32, then mean and std as fp64 operands rounded back to fp32, as to_tensors does).
//   One workgroup per (frame, band of output rows, slab of output columns): the input rows the band reads are resampled
//   horizontally into LDS, a chunk of rows at a time, and every thread keeps the vertical sums of its (at most 8) outputs in
//   registers across the chunks, so the LDS need is bounded whatever the downscale.  A thread of the horizontal pass makes
//   the three channels of one pixel (one coefficient load per tap for three byte loads, served by L1 / L2: neighbouring
//   lanes read neighbouring pixels); the f32 stores are coalesced along x.
// logits_to_u8_kernel: (B, 1, S, S) logits -> (B, H, W) u8, what save_predictions computes per image:
//   uint8(sigmoid(F.interpolate(res.float(), (H, W), mode="bilinear", align_corners=False)) * 255).  The resize is written
//   as torch's upsample_bilinear2d kernel computes it (source index, two-level lambda blend, with the FMAs its build
//   contracts to); each thread stores 16 consecutive output bytes with one 16-byte store.
// The *_ragged kernels are the same two computations for a batch of frames of different sizes: what depends on a frame's
//   size travels in a per-frame descriptor in device memory instead of in the kernel arguments (layout below).
#include "common.h"
#include "resample.h"

#include <math.h>
#include <string.h>

#include <vector>

namespace tramba {

constexpr int kFrThreads = 256;
constexpr int kFrMaxAcc = 8;              // vertical sums per thread: band * 3 * slab <= kFrThreads * kFrMaxAcc
constexpr int kFrLdsBytes = 32768;        // horizontally resampled rows staged per chunk
constexpr int kFrWantBlocks = 512;        // a band size that gives at least this many workgroups where it can
constexpr int kU8Threads = 256, kU8Bytes = 16;

// ---------------------------------------------------------------------------------------------- coefficient tables
// Word layout of a table (int32): xb[out_w][2] = {first input column, taps}, xk[out_w][kx] fixed-point weights, then
// yb[out_h][2], yk[out_h][ky], then lut[3][256] (f32 bits).  An axis whose size does not change gets one tap of weight
// 2^22 (acc >> 22 = px exactly: the pass is a copy, as Pillow skips it).
static double filter_support(int filter) { return filter == kFilterBicubic ? 2.0 : 1.0; }

// Pillow's bilinear (triangle) and bicubic (a = -0.5) kernels
static double filter_weight(int filter, double x)
{
#pragma clang fp contract(off)
    if (x < 0.0) x = -x;
    if (filter != kFilterBicubic) return x < 1.0 ? 1.0 - x : 0.0;
    const double a = -0.5;
    if (x < 1.0) return ((a + 2.0) * x - (a + 3.0)) * x * x + 1;
    if (x < 2.0) return (((x - 5) * x + 8) * x - 4) * a;
    return 0.0;
}

int resample_taps(int in, int out, int filter)
{
    if (in == out) return 1;
    const double scale = (double)in / out;
    const double fs = scale < 1.0 ? 1.0 : scale;
    return (int)ceil(filter_support(filter) * fs) * 2 + 1;
}

struct ResizeLayout {
    int kx, ky;
    size_t xb, xk, yb, yk, lut, words;
};

static ResizeLayout resize_layout(int in_h, int in_w, int out_h, int out_w)
{
    ResizeLayout L;
    L.kx = resample_taps(in_w, out_w, kFilterBilinear);
    L.ky = resample_taps(in_h, out_h, kFilterBilinear);
    L.xb = 0;
    L.xk = L.xb + 2 * (size_t)out_w;
    L.yb = L.xk + (size_t)out_w * L.kx;
    L.yk = L.yb + 2 * (size_t)out_h;
    L.lut = L.yk + (size_t)out_h * L.ky;
    L.words = L.lut + 3 * 256;
    return L;
}

bool frame_sizes_ok(int in_h, int in_w, int out_h, int out_w)
{
    return in_h >= 1 && in_w >= 1 && in_h <= TRAMBA_FRAME_MAX_DIM && in_w <= TRAMBA_FRAME_MAX_DIM && out_h >= 1 &&
           out_w >= 1 && out_h <= TRAMBA_FRAME_MAX_OUT && out_w <= TRAMBA_FRAME_MAX_OUT;
}

// One axis, Pillow's rule for 8-bit images (precompute_coeffs + normalize_coeffs_8bpc).  No contraction: `center - support`
// and the other sums must round as separate fp64 operations.
bool resample_axis(int in, int out, int filter, int ksize, int *bounds, int *coef)
{
#pragma clang fp contract(off)
    if (in == out) {
        for (int i = 0; i < out; ++i) {
            bounds[2 * i] = i;
            bounds[2 * i + 1] = 1;
            coef[i] = 1 << kPrecBits;
        }
        return true;
    }
    const double scale = (double)in / out;
    const double fs = scale < 1.0 ? 1.0 : scale;
    const double support = filter_support(filter) * fs;
    const double ss = 1.0 / fs;
    std::vector<double> w(ksize);
    for (int i = 0; i < out; ++i) {
        const double center = (i + 0.5) * scale;
        int xmin = (int)(center - support + 0.5);
        int xmax = (int)(center + support + 0.5);
        if (xmin < 0) xmin = 0;
        if (xmax > in) xmax = in;
        const int n = xmax - xmin;
        if (n < 1 || n > ksize) return false;
        double ww = 0.0;
        for (int j = 0; j < n; ++j) {
            w[j] = filter_weight(filter, ((double)(j + xmin) - center + 0.5) * ss);
            ww += w[j];
        }
        for (int j = 0; j < n; ++j)
            if (ww != 0.0) w[j] /= ww;
        for (int j = 0; j < ksize; ++j) {
            const double v = j < n ? w[j] * (double)(1 << kPrecBits) : 0.0;
            coef[(size_t)i * ksize + j] = j >= n ? 0 : (v < 0.0 ? (int)(-0.5 + v) : (int)(0.5 + v));
        }
        bounds[2 * i] = xmin;
        bounds[2 * i + 1] = n;
    }
    return true;
}

void normalise_lut(const double *mean, const double *std, float *lut)
{
#pragma clang fp contract(off)
    for (int c = 0; c < 3; ++c)
        for (int u = 0; u < 256; ++u) {
            const float f = (float)u / 255.0f;
            const float t = (float)((double)f - mean[c]);
            lut[c * 256 + u] = (float)((double)t / std[c]);
        }
}

// ---------------------------------------------------------------------------------------------- frames -> model input
__device__ __forceinline__ int clamp_u8(int acc)
{
    const int v = acc >> kPrecBits;            // acc >= 2^21 > 0: the weights are non-negative
    return v > 255 ? 255 : v;
}

// One workgroup's tile of frame blockIdx.z: `src` is that frame, `table` its coefficient table.  Shared by the uniform kernel
// (sizes in the arguments) and the ragged one (sizes in the frame's descriptor).
__device__ __forceinline__ void frames_tile(const unsigned char *__restrict__ src, const int *__restrict__ table,
                                            float *__restrict__ out, int W, int OH, int OW, int kx, int ky, int slab, int band,
                                            int chunk, int bgr)
{
    extern __shared__ unsigned char hrows[];   // [chunk][slab * 3]: input rows resampled along x, RGB interleaved
    __shared__ float lut[3 * 256];
    const int *xb = table, *xk = xb + 2 * (size_t)OW, *yb = xk + (size_t)OW * kx, *yk = yb + 2 * (size_t)OH;
    const float *tlut = reinterpret_cast<const float *>(yk + (size_t)OH * ky);
    for (int i = threadIdx.x; i < 3 * 256; i += kFrThreads) lut[i] = tlut[i];

    const int x0 = blockIdx.x * slab, sw = min(OW, x0 + slab) - x0;
    const int y0 = blockIdx.y * band, y1 = min(OH, y0 + band);
    const int b = blockIdx.z;
    const int rowlen = sw * 3;
    const int nout = (y1 - y0) * rowlen;       // outputs of the tile, ordered (row, channel, x)
    const int ylo = yb[2 * y0], yhi = yb[2 * (y1 - 1)] + yb[2 * (y1 - 1) + 1];   // bounds are monotone in the row

    int acc[kFrMaxAcc];
#pragma unroll
    for (int k = 0; k < kFrMaxAcc; ++k) acc[k] = 1 << (kPrecBits - 1);

    for (int c0 = ylo; c0 < yhi; c0 += chunk) {
        const int c1 = min(yhi, c0 + chunk);
        const int npx = (c1 - c0) * sw;            // (row, column) pairs: one thread makes the 3 channels of a pixel
        for (int o = threadIdx.x; o < npx; o += kFrThreads) {
            const int r = o / sw, xl = o - r * sw, x = x0 + xl;
            const int xmin = xb[2 * x], n = xb[2 * x + 1];
            const unsigned char *p = src + ((size_t)(c0 + r) * W + xmin) * 3;
            const int *k = xk + (size_t)x * kx;
            int s0 = 1 << (kPrecBits - 1), s1 = s0, s2 = s0;
#pragma unroll 4
            for (int j = 0; j < n; ++j) {
                const int kj = k[j];
                s0 += (int)p[3 * j] * kj;
                s1 += (int)p[3 * j + 1] * kj;
                s2 += (int)p[3 * j + 2] * kj;
            }
            unsigned char *h = hrows + r * rowlen + 3 * xl;
            h[0] = (unsigned char)clamp_u8(s0);
            h[1] = (unsigned char)clamp_u8(s1);
            h[2] = (unsigned char)clamp_u8(s2);
        }
        __syncthreads();
#pragma unroll
        for (int k = 0; k < kFrMaxAcc; ++k) {
            const int o = threadIdx.x + k * kFrThreads;
            if (o < nout) {
                const int r = o / rowlen, q = o - r * rowlen, c = q / sw, xl = q - c * sw;
                const int y = y0 + r, ymin = yb[2 * y], ymax = ymin + yb[2 * y + 1];
                const int j0 = max(ymin, c0), j1 = min(ymax, c1);
                const int *wk = yk + (size_t)y * ky;
                const int col = 3 * xl + (bgr ? 2 - c : c);
                int s = acc[k];
                for (int j = j0; j < j1; ++j) s += (int)hrows[(j - c0) * rowlen + col] * wk[j - ymin];
                acc[k] = s;
            }
        }
        __syncthreads();
    }
#pragma unroll
    for (int k = 0; k < kFrMaxAcc; ++k) {
        const int o = threadIdx.x + k * kFrThreads;
        if (o < nout) {
            const int r = o / rowlen, q = o - r * rowlen, c = q / sw, xl = q - c * sw;
            out[((size_t)b * 3 + c) * OH * OW + (size_t)(y0 + r) * OW + x0 + xl] = lut[c * 256 + clamp_u8(acc[k])];
        }
    }
}

__global__ __launch_bounds__(kFrThreads) void frames_to_input_kernel(const unsigned char *__restrict__ frames,
                                                                     const int *__restrict__ table, float *__restrict__ out,
                                                                     int H, int W, int OH, int OW, int kx, int ky, int slab,
                                                                     int band, int chunk, int bgr)
{
    frames_tile(frames + (size_t)blockIdx.z * H * W * 3, table, out, W, OH, OW, kx, ky, slab, band, chunk, bgr);
}

// A packed batch of frames of different sizes (one flat u8 buffer): batch descriptors of TRAMBA_FRAMES_DESC_WORDS int64
// words, then the coefficient tables (the tramba_resize_table words, one per distinct frame size) and the frames (h, w, 3)
// at the byte offsets the descriptors name.  Both ragged launches depend on (batch, S) and the output capacity only, so one
// captured graph serves every mix of sizes.
enum {
    kRgFrame = 0,       // byte offset of the (h, w, 3) frame in the packed buffer
    kRgH,
    kRgW,
    kRgTable,           // byte offset of the tramba_resize_table words for (h, w) -> (S, S), a multiple of 4
    kRgKx,              // taps per output column and per output row of that table
    kRgKy,
    kRgOut,             // byte offset of the (h, w) map in the output buffer, a multiple of 16
    kRgRh,              // (float)S / (float)h and (float)S / (float)w as fp32 bits: torch's area_pixel_compute_scale, made on
    kRgRw,              // the host as the uniform entry makes it, so no device-side division can round differently
    kRgUsed
};
static_assert(kRgUsed <= TRAMBA_FRAMES_DESC_WORDS, "descriptor layout");

__device__ __forceinline__ const long long *ragged_desc(const unsigned char *packed, int b)
{
    return reinterpret_cast<const long long *>(packed) + (size_t)b * TRAMBA_FRAMES_DESC_WORDS;
}

__global__ __launch_bounds__(kFrThreads) void frames_to_input_ragged_kernel(const unsigned char *__restrict__ packed,
                                                                            float *__restrict__ out, int S, int slab, int band,
                                                                            int chunk, int bgr)
{
    const long long *d = ragged_desc(packed, blockIdx.z);
    frames_tile(packed + d[kRgFrame], reinterpret_cast<const int *>(packed + d[kRgTable]), out, (int)d[kRgW], S, S,
                (int)d[kRgKx], (int)d[kRgKy], slab, band, chunk, bgr);
}

// ---------------------------------------------------------------------------------------------- logits -> u8 maps
// torch's upsample_bilinear2d arithmetic as its build compiles it: its source is plain `a * b + c` expressions and the HIP
// compiler contracts them by default, the product written first going into the FMA.  Written out here with explicit fmaf
// and contraction off, so this file's compiler cannot pick another pairing (pre-sigmoid floats compared on the GPU).
// area_pixel_compute_source_index (align_corners=False, not cubic): max(scale * (dst + 0.5) - 0.5, 0)
__device__ __forceinline__ float source_index(float scale, int dst)
{
#pragma clang fp contract(off)
    const float src = __builtin_fmaf(scale, (float)dst + 0.5f, -0.5f);
    return src < 0.f ? 0.f : src;
}

template <typename T>
__device__ __forceinline__ unsigned char saliency_u8(const T *__restrict__ img, int IH, int IW, int y, int x, float rh,
                                                     float rw, bool copy)
{
#pragma clang fp contract(off)
    float val;
    if (copy) {
        val = Cvt<T>::to_f(img[(size_t)y * IW + x]);
    } else {
        const float h1r = source_index(rh, y);
        const int h1 = (int)h1r;
        const int h1p = h1 < IH - 1 ? 1 : 0;
        const float h1lambda = h1r - h1;
        const float h0lambda = 1.f - h1lambda;
        const float w1r = source_index(rw, x);
        const int w1 = (int)w1r;
        const int w1p = w1 < IW - 1 ? 1 : 0;
        const float w1lambda = w1r - w1;
        const float w0lambda = 1.f - w1lambda;
        const T *r0 = img + (size_t)h1 * IW + w1, *r1 = img + (size_t)(h1 + h1p) * IW + w1;
        // h0lambda * (w0lambda * a + w1lambda * b) + h1lambda * (w0lambda * c + w1lambda * d)
        const float top = __builtin_fmaf(w0lambda, Cvt<T>::to_f(r0[0]), w1lambda * Cvt<T>::to_f(r0[w1p]));
        const float bot = __builtin_fmaf(w0lambda, Cvt<T>::to_f(r1[0]), w1lambda * Cvt<T>::to_f(r1[w1p]));
        val = __builtin_fmaf(h0lambda, top, h1lambda * bot);
    }
    const float sg = 1.f / (1.f + expf(-val));         // IEEE division and the library expf, as torch.sigmoid
    return (unsigned char)(int)(sg * 255.f);             // in [0, 255]: truncation, as .to(torch.uint8)
}

template <typename T>
__global__ __launch_bounds__(kU8Threads) void logits_to_u8_kernel(const T *__restrict__ logits, unsigned char *__restrict__ out,
                                                                  int IH, int IW, int H, int W, size_t total, float rh,
                                                                  float rw)
{
    const size_t base = ((size_t)blockIdx.x * kU8Threads + threadIdx.x) * kU8Bytes;
    if (base >= total) return;
    const bool copy = IH == H && IW == W;              // torch's special case: sizes equal, values copied
    const size_t plane = (size_t)H * W;
    size_t b = base / plane;
    const size_t rem = base - b * plane;
    int y = (int)(rem / W), x = (int)(rem - (size_t)y * W);
    unsigned char v[kU8Bytes];
#pragma unroll
    for (int i = 0; i < kU8Bytes; ++i) {
        v[i] = base + i < total ? saliency_u8(logits + b * IH * IW, IH, IW, y, x, rh, rw, copy) : 0;
        if (++x == W) {
            x = 0;
            if (++y == H) {
                y = 0;
                ++b;
            }
        }
    }
    if (base + kU8Bytes <= total) {
        Pack<unsigned char, kU8Bytes> pk;
#pragma unroll
        for (int i = 0; i < kU8Bytes; ++i) pk.v[i] = v[i];
        *reinterpret_cast<Pack<unsigned char, kU8Bytes> *>(out + base) = pk;
    } else {
        for (int i = 0; base + i < total; ++i) out[base + i] = v[i];
    }
}

// The grid covers the output buffer's CAPACITY, 16 bytes per thread.  The map offsets increase and are 16-byte aligned, so a
// thread's 16 bytes belong to at most one map: the workgroup finds the last map that starts at or before its first byte by
// binary search (as adam_kernel finds its tensor), a thread steps on from there (short maps: several per workgroup), and
// bytes between two maps or past the last one are left alone.
template <typename T>
__global__ __launch_bounds__(kU8Threads) void logits_to_u8_ragged_kernel(const T *__restrict__ logits,
                                                                         const unsigned char *__restrict__ packed,
                                                                         unsigned char *__restrict__ out, int batch, int S)
{
    const size_t first = (size_t)blockIdx.x * kU8Threads * kU8Bytes;
    const long long *last = ragged_desc(packed, batch - 1);
    if (first >= (size_t)(last[kRgOut] + last[kRgH] * last[kRgW])) return;   // past the batch's last byte
    int lo = 0, hi = batch;
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if ((size_t)ragged_desc(packed, mid)[kRgOut] <= first) lo = mid; else hi = mid;
    }
    const size_t base = first + (size_t)threadIdx.x * kU8Bytes;
    while (lo + 1 < batch && (size_t)ragged_desc(packed, lo + 1)[kRgOut] <= base) ++lo;
    const long long *d = ragged_desc(packed, lo);
    const size_t off = (size_t)d[kRgOut];
    const int H = (int)d[kRgH], W = (int)d[kRgW];
    const size_t total = (size_t)H * W;
    if (base < off || base - off >= total) return;
    const size_t at = base - off;
    const float rh = __uint_as_float((unsigned)d[kRgRh]), rw = __uint_as_float((unsigned)d[kRgRw]);
    const bool copy = S == H && S == W;
    const T *img = logits + (size_t)lo * S * S;
    int y = (int)(at / W), x = (int)(at - (size_t)y * W);
    unsigned char v[kU8Bytes];
#pragma unroll
    for (int i = 0; i < kU8Bytes; ++i) {
        v[i] = at + i < total ? saliency_u8(img, S, S, y, x, rh, rw, copy) : 0;
        if (++x == W) {
            x = 0;
            ++y;
        }
    }
    if (at + kU8Bytes <= total) {
        Pack<unsigned char, kU8Bytes> pk;
#pragma unroll
        for (int i = 0; i < kU8Bytes; ++i) pk.v[i] = v[i];
        *reinterpret_cast<Pack<unsigned char, kU8Bytes> *>(out + base) = pk;
    } else {
        for (int i = 0; at + i < total; ++i) out[base + i] = v[i];
    }
}

static unsigned f32_bits(float f)
{
    unsigned u;
    memcpy(&u, &f, sizeof u);
    return u;
}

// The host copy of a packed batch's descriptors against the buffer sizes; `parts` selects the input half (frames and
// tables inside packed_bytes), the output half (maps inside out_capacity), or both.
static int ragged_check(const char *who, const int64_t *desc, int batch, int size, size_t packed_bytes, size_t out_capacity,
                        int parts)
{
    TRAMBA_CHECK(desc, "%s: null pointer", who);
    TRAMBA_CHECK(batch >= 1 && batch <= 65535, "%s: batch %d outside 1 .. 65535", who, batch);
    TRAMBA_CHECK(size >= 3 && size <= TRAMBA_FRAME_MAX_OUT, "%s: output size %d outside 3 .. %d", who, size,
                 TRAMBA_FRAME_MAX_OUT);
    TRAMBA_CHECK(parts >= 1 && parts <= (TRAMBA_RAGGED_IN | TRAMBA_RAGGED_OUT), "%s: parts %d selects nothing known", who,
                 parts);
    const uint64_t head = (uint64_t)batch * TRAMBA_FRAMES_DESC_WORDS * 8;
    if (parts & TRAMBA_RAGGED_IN)
        TRAMBA_CHECK(packed_bytes >= head, "%s: %zu packed bytes do not hold the descriptor area of %d frames", who,
                     packed_bytes, batch);
    int64_t prev = -1, end = 0;                 // the previous map's offset and end
    for (int b = 0; b < batch; ++b) {
        const int64_t *d = desc + (size_t)b * TRAMBA_FRAMES_DESC_WORDS;
        const int64_t h = d[kRgH], w = d[kRgW];
        TRAMBA_CHECK(h >= 1 && w >= 1 && h <= TRAMBA_FRAME_MAX_DIM && w <= TRAMBA_FRAME_MAX_DIM,
                     "%s: frame %d is %lldx%lld, a side outside 1 .. %d", who, b, (long long)h, (long long)w,
                     TRAMBA_FRAME_MAX_DIM);
        if (parts & TRAMBA_RAGGED_IN) {
            const ResizeLayout L = resize_layout((int)h, (int)w, size, size);
            const int64_t fo = d[kRgFrame], to = d[kRgTable];
            TRAMBA_CHECK(fo >= (int64_t)head && to >= (int64_t)head,
                         "%s: frame %d: offsets %lld / %lld lie inside the descriptor area of %llu bytes", who, b,
                         (long long)fo, (long long)to, (unsigned long long)head);
            TRAMBA_CHECK((uint64_t)fo <= packed_bytes && (uint64_t)(h * w * 3) <= packed_bytes - (uint64_t)fo &&
                             (uint64_t)to <= packed_bytes && (uint64_t)L.words * 4 <= packed_bytes - (uint64_t)to,
                         "%s: frame %d or its table lies outside the %zu packed bytes", who, b, packed_bytes);
            TRAMBA_CHECK(to % 4 == 0, "%s: frame %d: table offset %lld is not aligned to 4 bytes", who, b, (long long)to);
            TRAMBA_CHECK(d[kRgKx] == L.kx && d[kRgKy] == L.ky,
                         "%s: frame %d: taps %lld / %lld, the table of %lldx%lld -> %d has %d / %d", who, b,
                         (long long)d[kRgKx], (long long)d[kRgKy], (long long)h, (long long)w, size, L.kx, L.ky);
        }
        if (parts & TRAMBA_RAGGED_OUT) {
            const int64_t oo = d[kRgOut];
            TRAMBA_CHECK(oo > prev, "%s: map %d: output offset %lld is not increasing", who, b, (long long)oo);
            TRAMBA_CHECK(oo % 16 == 0, "%s: map %d: output offset %lld is not aligned to 16 bytes", who, b, (long long)oo);
            TRAMBA_CHECK(oo >= end, "%s: map %d at %lld would overlap map %d, which ends at %lld", who, b, (long long)oo, b - 1,
                         (long long)end);
            TRAMBA_CHECK((uint64_t)oo <= out_capacity && (uint64_t)(h * w) <= out_capacity - (uint64_t)oo,
                         "%s: map %d ends at %lld, above the capacity of %zu bytes", who, b, (long long)(oo + h * w),
                         out_capacity);
            TRAMBA_CHECK(d[kRgRh] == (int64_t)f32_bits((float)size / (float)h) &&
                             d[kRgRw] == (int64_t)f32_bits((float)size / (float)w),
                         "%s: map %d: the scale words are not the fp32 bits of %d / %lld and %d / %lld", who, b, size,
                         (long long)h, size, (long long)w);
            prev = oo;
            end = oo + h * w;
        }
    }
    return TRAMBA_OK;
}

}  // namespace tramba

using namespace tramba;

extern "C" size_t tramba_resize_table_words(int in_h, int in_w, int out_h, int out_w)
{
    return frame_sizes_ok(in_h, in_w, out_h, out_w) ? resize_layout(in_h, in_w, out_h, out_w).words : 0;
}

extern "C" int tramba_resize_table(int in_h, int in_w, int out_h, int out_w, const double *mean, const double *std,
                                   int *table, size_t words)
{
    TRAMBA_CHECK(table && mean && std, "resize_table: null pointer");
    TRAMBA_CHECK(frame_sizes_ok(in_h, in_w, out_h, out_w),
                 "resize_table: %dx%d -> %dx%d outside 1 .. %d per input side, 1 .. %d per output side", in_h, in_w, out_h,
                 out_w, TRAMBA_FRAME_MAX_DIM, TRAMBA_FRAME_MAX_OUT);
    const ResizeLayout L = resize_layout(in_h, in_w, out_h, out_w);
    TRAMBA_CHECK(words >= L.words, "resize_table: %zu words given, %zu needed", words, L.words);
    for (int c = 0; c < 3; ++c) TRAMBA_CHECK(std[c] != 0.0, "resize_table: std[%d] is zero", c);
    TRAMBA_CHECK(resample_axis(in_w, out_w, kFilterBilinear, L.kx, table + L.xb, table + L.xk) &&
                 resample_axis(in_h, out_h, kFilterBilinear, L.ky, table + L.yb, table + L.yk), "resize_table: tap count out of range");
    normalise_lut(mean, std, reinterpret_cast<float *>(table + L.lut));
    return TRAMBA_OK;
}

// A workgroup takes `band` output rows x `slab` output columns of one frame: at most kFrThreads * kFrMaxAcc outputs.  The
// geometry is a function of (batch, output size) only, which is what lets the ragged entry share it.
struct FrameGeometry {
    int slab, band, chunk;
    dim3 grid;
    size_t lds;
};

static FrameGeometry frame_geometry(int batch, int out_h, int out_w)
{
    FrameGeometry g;
    const int slab_max = kFrThreads * kFrMaxAcc / 3, nslab = (out_w + slab_max - 1) / slab_max;
    g.slab = (out_w + nslab - 1) / nslab;
    const int band_max = kFrThreads * kFrMaxAcc / (3 * g.slab);
    const int band = (int)((long long)out_h * nslab * batch / kFrWantBlocks);
    g.band = band < 1 ? 1 : (band > band_max ? band_max : band);
    g.chunk = kFrLdsBytes / (3 * g.slab);        // >= 16 input rows per LDS chunk
    g.grid = dim3(nslab, (out_h + g.band - 1) / g.band, batch);
    g.lds = (size_t)g.chunk * 3 * g.slab;
    return g;
}

extern "C" int tramba_frames_to_input(const unsigned char *frames, const int *table, float *out, int batch, int h, int w,
                                      int out_h, int out_w, int bgr, void *stream)
{
    TRAMBA_CHECK(frames && table && out, "frames_to_input: null pointer");
    TRAMBA_CHECK(batch >= 1 && batch <= 65535, "frames_to_input: batch %d outside 1 .. 65535", batch);
    TRAMBA_CHECK(frame_sizes_ok(h, w, out_h, out_w),
                 "frames_to_input: %dx%d -> %dx%d outside 1 .. %d per frame side, 1 .. %d per output side", h, w, out_h,
                 out_w, TRAMBA_FRAME_MAX_DIM, TRAMBA_FRAME_MAX_OUT);
    const ResizeLayout L = resize_layout(h, w, out_h, out_w);
    const FrameGeometry g = frame_geometry(batch, out_h, out_w);
    hipLaunchKernelGGL(frames_to_input_kernel, g.grid, dim3(kFrThreads), g.lds, (hipStream_t)stream, frames, table, out, h, w,
                       out_h, out_w, L.kx, L.ky, g.slab, g.band, g.chunk, bgr ? 1 : 0);
    TRAMBA_LAUNCH_CHECK();
    return TRAMBA_OK;
}

extern "C" int tramba_logits_to_u8(const void *logits, unsigned char *out, int batch, int in_h, int in_w, int h, int w,
                                   int dtype, void *stream)
{
    TRAMBA_CHECK(logits && out, "logits_to_u8: null pointer");
    TRAMBA_CHECK(batch >= 1 && batch <= 65535 && in_h >= 1 && in_w >= 1 && in_h <= TRAMBA_FRAME_MAX_OUT &&
                     in_w <= TRAMBA_FRAME_MAX_OUT && h >= 1 && w >= 1 && h <= TRAMBA_FRAME_MAX_DIM && w <= TRAMBA_FRAME_MAX_DIM,
                 "logits_to_u8: (%d, %d, %d) -> %dx%d outside 1 .. %d per logit side, 1 .. %d per map side", batch, in_h,
                 in_w, h, w, TRAMBA_FRAME_MAX_OUT, TRAMBA_FRAME_MAX_DIM);
    const size_t total = (size_t)batch * h * w;
    const size_t threads = (total + kU8Bytes - 1) / kU8Bytes;
    TRAMBA_CHECK((threads + kU8Threads - 1) / kU8Threads <= 0x7fffffff, "logits_to_u8: %zu output bytes are too many", total);
    const dim3 grid((unsigned)((threads + kU8Threads - 1) / kU8Threads));
    const float rh = (float)in_h / (float)h, rw = (float)in_w / (float)w;   // torch's area_pixel_compute_scale, on the host
    TRAMBA_DISPATCH_DTYPE(dtype, T,
                          hipLaunchKernelGGL(logits_to_u8_kernel<T>, grid, dim3(kU8Threads), 0, (hipStream_t)stream,
                                             reinterpret_cast<const T *>(logits), out, in_h, in_w, h, w, total, rh, rw));
    TRAMBA_LAUNCH_CHECK();
    return TRAMBA_OK;
}

extern "C" int tramba_frames_ragged_check(const int64_t *desc_host, int batch, int size, size_t packed_bytes,
                                          size_t out_capacity, int parts)
{
    return ragged_check("frames_ragged_check", desc_host, batch, size, packed_bytes, out_capacity, parts);
}

extern "C" int tramba_frames_to_input_ragged(const unsigned char *packed, const int64_t *desc_host, size_t packed_bytes,
                                             float *out, int batch, int size, int bgr, void *stream)
{
    TRAMBA_CHECK(packed && desc_host && out, "frames_to_input_ragged: null pointer");
    TRAMBA_CHECK(aligned16(packed), "frames_to_input_ragged: the packed buffer is not aligned to 16 bytes");
    const int rc = ragged_check("frames_to_input_ragged", desc_host, batch, size, packed_bytes, 0, TRAMBA_RAGGED_IN);
    if (rc != TRAMBA_OK) return rc;
    const FrameGeometry g = frame_geometry(batch, size, size);
    hipLaunchKernelGGL(frames_to_input_ragged_kernel, g.grid, dim3(kFrThreads), g.lds, (hipStream_t)stream, packed, out, size,
                       g.slab, g.band, g.chunk, bgr ? 1 : 0);
    TRAMBA_LAUNCH_CHECK();
    return TRAMBA_OK;
}

extern "C" int tramba_logits_to_u8_ragged(const void *logits, const unsigned char *packed, const int64_t *desc_host,
                                          unsigned char *out, size_t out_capacity, int batch, int size, int dtype, void *stream)
{
    TRAMBA_CHECK(logits && packed && desc_host && out, "logits_to_u8_ragged: null pointer");
    TRAMBA_CHECK(aligned16(packed) && aligned16(out),
                 "logits_to_u8_ragged: the packed or the output buffer is not aligned to 16 bytes");
    const int rc = ragged_check("logits_to_u8_ragged", desc_host, batch, size, 0, out_capacity, TRAMBA_RAGGED_OUT);
    if (rc != TRAMBA_OK) return rc;
    const size_t per_block = (size_t)kU8Threads * kU8Bytes, blocks = (out_capacity + per_block - 1) / per_block;
    TRAMBA_CHECK(blocks <= 0x7fffffff, "logits_to_u8_ragged: a capacity of %zu bytes is too large", out_capacity);
    TRAMBA_DISPATCH_DTYPE(dtype, T,
                          hipLaunchKernelGGL(logits_to_u8_ragged_kernel<T>, dim3((unsigned)blocks), dim3(kU8Threads), 0,
                                             (hipStream_t)stream, reinterpret_cast<const T *>(logits), packed, out, batch, size));
    TRAMBA_LAUNCH_CHECK();
    return TRAMBA_OK;
}
