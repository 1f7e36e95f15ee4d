// The training transform on the device: uint8 image / mask pairs of any size in, train batches out, bit for bit what
// data.get_transform(S, "train") gives for the same numpy draws (static resize, scale-crop, mirror, rotation, the three
// enhancers in the sample's order, to_tensors).  The draws are made on the host (tramba_amd/augment.py); a batch arrives as
// ONE packed u8 buffer whose first batch * TRAMBA_AUG_DESC_WORDS int64 words are the per-sample descriptors.
//
// Four launches per batch, each for the whole batch (workspace: A, T, G below; each sample's (S, S) pixels are 4 bytes,
// R, G, B and the mask):
//   augment_resize_kernel     original size -> A (S, S, 4): Pillow's bilinear resample for the image (frames_to_input's
//                             band / slab structure, u8 results instead of the f32 table), nearest for the mask (Pillow's
//                             scale-affine path: an index per output row and column);
//   augment_scale_rows_kernel samples with a scale-crop: the horizontal bicubic pass A -> T (S, R, 4), u8 results;
//   augment_geometry_kernel   one gather per output pixel -> G (S, S, 4): the rotation's 16.16 fixed-point map (with its
//                             centre crop folded in), the mirror, the pad / centre crop of the scale and the vertical bicubic
//                             pass over T (or A when there is no scale);
//   augment_enhance_kernel    one workgroup per sample: contrast / brightness / sharpness in the sample's order, ping-pong
//                             between G and A, the last pass writing the f32 image (normalisation table) and label (u / 255).
#include "common.h"
#include "resample.h"

#include <math.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

namespace tramba {

constexpr int kAgThreads = 256;
constexpr int kAgMaxAcc = 8;              // vertical sums per thread of the static resize (as frames_to_input)
constexpr int kAgLdsBytes = 32768;
constexpr int kAgWantBlocks = 512;
constexpr int kEnhThreads = 1024;

// descriptor words (int64), TRAMBA_AUG_DESC_WORDS per sample
enum {
    kDImg = 0,          // byte offset of the (h, w, 3) RGB image in the packed buffer
    kDMask,             // byte offset of the (h, w) mask
    kDH,
    kDW,
    kDSrcTable,         // device address of the library's source table for (h, w) -> (S, S)
    kDR,                // scale-crop: resampled side R (0: none, or R == S, Pillow's copy)
    kDOff,              // (R - S) // 2: the centre crop's origin in the R x R image (negative: padded)
    kDScaleTable,       // device address of the S -> R bicubic axis table
    kDTaps,             // its taps per output sample
    kDMirror,           // 1: left-right flip
    kDRot,              // 1: rotation (coefficients below), 0: none
    kDRotCoef,          // 6 words: A0, A1, A2, A3, A4, A5 (16.16): src = (A0 x + A1 y + A2, A3 x + A4 y + A5) >> 16
    kDEnhCount = kDRotCoef + 6,
    kDEnhOp,            // 3 words: TRAMBA_AUG_CONTRAST / _BRIGHTNESS / _SHARPNESS in the order they apply
    kDEnhFactor = kDEnhOp + 3,   // 3 words: the blend factors as fp32 bits
    kDDegrees = kDEnhFactor + 3, // the drawn angle in [0, 360) (host bookkeeping; the kernels read kDRot*)
    kDUsed
};
static_assert(kDUsed <= TRAMBA_AUG_DESC_WORDS, "descriptor layout");

// size table (int32 words) of one output side S
constexpr int kStNorm = 0;                // [3][256] f32: the image's normalisation table
constexpr int kStMask = 768;              // [256] f32: u / 255 (the label)
constexpr int kStSmooth = 1024;           // [9] f32: ImageFilter.SMOOTH normalised as Pillow does (kernel / 13 in fp32)
constexpr int kStRange = 1040;            // lo, hi: the R the table covers
constexpr int kStIndex = 1042;            // [hi - lo + 1]: word offset of each R's bicubic axis table (0 for R == S)

static int scale_lo(int S) { return (3 * S) / 4; }            // floor(0.75 S) <= round(S f) for f in [0.75, 1.25)
static int scale_hi(int S) { return (5 * S + 3) / 4; }        // ceil(1.25 S)
static bool aug_size_ok(int S) { return S >= 3 && S <= TRAMBA_FRAME_MAX_OUT; }

// ---------------------------------------------------------------------------------------------- host tables
// Pillow's resize(NEAREST) for 8-bit images goes through ImagingScaleAffine: xo = a * 0.5, then xo += a per output
// sample, accumulated in fp64, and the source index is (int)xo (-1 for xo < 0, out of range: the fill value 0).
static void nearest_axis(int in, int out, int *idx)
{
#pragma clang fp contract(off)
    if (in == out) {                          // Pillow copies the image
        for (int i = 0; i < out; ++i) idx[i] = i;
        return;
    }
    const double a = (double)in / out;
    double xo = a * 0.5;
    for (int i = 0; i < out; ++i) {
        const int xin = xo < 0.0 ? -1 : (int)xo;
        idx[i] = xin >= 0 && xin < in ? xin : -1;
        xo += a;
    }
}

// Source table of (h, w) -> (S, S): {kx, ky, 0, 0}, the tramba_resize_table words (bilinear bounds and weights; its
// normalisation table is not read here), then the nearest indices nx[S], ny[S].
static size_t source_words(int h, int w, int S) { return 4 + tramba_resize_table_words(h, w, S, S) + 2 * (size_t)S; }

static size_t size_words(int S)
{
    size_t words = kStIndex + (size_t)(scale_hi(S) - scale_lo(S) + 1);
    for (int R = scale_lo(S); R <= scale_hi(S); ++R)
        if (R != S) words += 2 * (size_t)R + (size_t)R * resample_taps(S, R, kFilterBicubic);
    return words;
}

// Python's round(v, 15): the correctly rounded decimal with 15 fractional digits, read back
static double round15(double v)
{
    char buf[64];
    snprintf(buf, sizeof buf, "%.15f", v);
    return strtod(buf, nullptr);
}

// Image.rotate(deg, expand=True) on an S x S image then the centre crop back to S x S, as Pillow computes it: the matrix in
// Python fp64 (Image.rotate), then affine_fixed's 16.16 coefficients (FIX(v) = FLOOR(v 65536 + 0.5)), the crop origin
// folded into the constant terms.  False when Pillow would not take the fixed-point path.
static bool rotation_coefficients(int S, int degrees, int *coef)
{
#pragma clang fp contract(off)
    double angle = fmod((double)degrees, 360.0);
    if (angle < 0.0) angle += 360.0;
    if (angle == 0.0 || angle == 90.0 || angle == 180.0 || angle == 270.0) return false;   // Pillow's transpose shortcuts
    const double w = S, h = S, cx = w / 2, cy = h / 2;
    const double rad = -(angle * (M_PI / 180.0));
    double m[6] = {round15(cos(rad)), round15(sin(rad)), 0.0, round15(-sin(rad)), round15(cos(rad)), 0.0};
    auto tx = [&](double x, double y) { return m[0] * x + m[1] * y + m[2]; };
    auto ty = [&](double x, double y) { return m[3] * x + m[4] * y + m[5]; };
    {
        const double c = tx(-cx - 0, -cy - 0), f = ty(-cx - 0, -cy - 0);
        m[2] = c + cx;
        m[5] = f + cy;
    }
    const double px[4] = {0, w, w, 0}, py[4] = {0, 0, h, h};
    double xmin = 1e300, xmax = -1e300, ymin = 1e300, ymax = -1e300;
    for (int i = 0; i < 4; ++i) {
        const double x = tx(px[i], py[i]), y = ty(px[i], py[i]);
        xmin = fmin(xmin, x), xmax = fmax(xmax, x), ymin = fmin(ymin, y), ymax = fmax(ymax, y);
    }
    const int nw = (int)(ceil(xmax) - floor(xmin)), nh = (int)(ceil(ymax) - floor(ymin));
    {
        const double x = -(nw - w) / 2.0, y = -(nh - h) / 2.0;
        const double c = tx(x, y), f = ty(x, y);
        m[2] = c;
        m[5] = f;
    }
    if (nw < S || nh < S) return false;
    auto fixed_ok = [&](double x, double y) {
        return fabs(x * m[0] + y * m[1] + m[2]) < 32768.0 && fabs(x * m[3] + y * m[4] + m[5]) < 32768.0;
    };
    if (!(fixed_ok(0, 0) && fixed_ok(nw, nh) && fixed_ok(0, nh) && fixed_ok(nw, 0))) return false;
    auto fix = [](double v) {
        const double t = v * 65536.0 + 0.5;
        return t < 0.0 ? (long long)floor(t) : (long long)t;
    };
    const long long a0 = fix(m[0]), a1 = fix(m[1]), a3 = fix(m[3]), a4 = fix(m[4]);
    const long long a2 = fix(m[2] + m[0] * 0.5 + m[1] * 0.5), a5 = fix(m[5] + m[3] * 0.5 + m[4] * 0.5);
    const long long bx = (nw - S) / 2, by = (nh - S) / 2;     // _centre_box of the crop (both >= 0)
    coef[0] = (int)a0;
    coef[1] = (int)a1;
    coef[2] = (int)(a2 + bx * a0 + by * a1);
    coef[3] = (int)a3;
    coef[4] = (int)a4;
    coef[5] = (int)(a5 + bx * a3 + by * a4);
    return true;
}

// ---------------------------------------------------------------------------------------------- device helpers
__device__ __forceinline__ int clip_pos(int acc)        // non-negative weights (bilinear)
{
    const int v = acc >> kPrecBits;
    return v > 255 ? 255 : v;
}

__device__ __forceinline__ int clip_any(int acc)        // Pillow's clip8: floor(acc / 2^22) clamped at both ends
{
    const int v = acc >> kPrecBits;
    return v < 0 ? 0 : (v > 255 ? 255 : v);
}

__device__ __forceinline__ const long long *sample_desc(const unsigned char *packed, int b)
{
    return reinterpret_cast<const long long *>(packed) + (size_t)b * TRAMBA_AUG_DESC_WORDS;
}

// ---------------------------------------------------------------------------------------------- (a) static resize
__global__ __launch_bounds__(kAgThreads) void augment_resize_kernel(const unsigned char *__restrict__ packed,
                                                                    unsigned char *__restrict__ A, int S, int slab, int band,
                                                                    int chunk)
{
    extern __shared__ unsigned char hrows[];   // [chunk][slab * 3]
    const int b = blockIdx.z;
    const long long *d = sample_desc(packed, b);
    const int H = (int)d[kDH], W = (int)d[kDW];
    const int *tab = reinterpret_cast<const int *>(d[kDSrcTable]);
    const int kx = tab[0], ky = tab[1];
    const int *xb = tab + 4, *xk = xb + 2 * (size_t)S, *yb = xk + (size_t)S * kx, *yk = yb + 2 * (size_t)S;
    const int *nx = yk + (size_t)S * ky + 3 * 256, *ny = nx + S;
    const unsigned char *src = packed + d[kDImg], *msrc = packed + d[kDMask];
    unsigned char *dst = A + (size_t)b * S * S * 4;

    const int x0 = blockIdx.x * slab, sw = min(S, x0 + slab) - x0;
    const int y0 = blockIdx.y * band, y1 = min(S, y0 + band);
    if (sw <= 0 || y0 >= S) return;
    const int rowlen = sw * 3;
    const int nout = (y1 - y0) * rowlen;
    const int ylo = yb[2 * y0], yhi = yb[2 * (y1 - 1)] + yb[2 * (y1 - 1) + 1];

    int acc[kAgMaxAcc];
#pragma unroll
    for (int k = 0; k < kAgMaxAcc; ++k) acc[k] = 1 << (kPrecBits - 1);

    for (int c0 = ylo; c0 < yhi; c0 += chunk) {
        const int c1 = min(yhi, c0 + chunk);
        const int npx = (c1 - c0) * sw;
        for (int o = threadIdx.x; o < npx; o += kAgThreads) {
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
            h[0] = (unsigned char)clip_pos(s0);
            h[1] = (unsigned char)clip_pos(s1);
            h[2] = (unsigned char)clip_pos(s2);
        }
        __syncthreads();
#pragma unroll
        for (int k = 0; k < kAgMaxAcc; ++k) {
            const int o = threadIdx.x + k * kAgThreads;
            if (o < nout) {
                const int r = o / rowlen, q = o - r * rowlen;
                const int y = y0 + r, ymin = yb[2 * y], ymax = ymin + yb[2 * y + 1];
                const int j0 = max(ymin, c0), j1 = min(ymax, c1);
                const int *wk = yk + (size_t)y * ky;
                int s = acc[k];
                for (int j = j0; j < j1; ++j) s += (int)hrows[(j - c0) * rowlen + q] * wk[j - ymin];
                acc[k] = s;
            }
        }
        __syncthreads();
    }
#pragma unroll
    for (int k = 0; k < kAgMaxAcc; ++k) {
        const int o = threadIdx.x + k * kAgThreads;
        if (o < nout) {
            const int r = o / rowlen, q = o - r * rowlen, xl = q / 3, c = q - xl * 3;
            dst[((size_t)(y0 + r) * S + x0 + xl) * 4 + c] = (unsigned char)clip_pos(acc[k]);
        }
    }
    // the mask of the same tile: nearest
    for (int o = threadIdx.x; o < (y1 - y0) * sw; o += kAgThreads) {
        const int r = o / sw, xl = o - r * sw, y = y0 + r, x = x0 + xl;
        const int ix = nx[x], iy = ny[y];
        dst[((size_t)y * S + x) * 4 + 3] = ix >= 0 && iy >= 0 ? msrc[(size_t)iy * W + ix] : 0;
    }
}

// ---------------------------------------------------------------------------------------------- (b) scale and geometry
__global__ __launch_bounds__(kAgThreads) void augment_scale_rows_kernel(const unsigned char *__restrict__ packed,
                                                                        const uchar4 *__restrict__ A, uchar4 *__restrict__ T,
                                                                        int S, int RS)
{
    const int b = blockIdx.y;
    const long long *d = sample_desc(packed, b);
    const int R = (int)d[kDR];
    const int o = blockIdx.x * kAgThreads + threadIdx.x;
    if (R == 0 || o >= S * R) return;
    const int y = o / R, u = o - y * R;
    const int *tab = reinterpret_cast<const int *>(d[kDScaleTable]);
    const int taps = (int)d[kDTaps];
    const int xmin = tab[2 * u], n = tab[2 * u + 1];
    const int *k = tab + 2 * (size_t)R + (size_t)u * taps;
    const uchar4 *row = A + ((size_t)b * S + y) * S + xmin;
    int s0 = 1 << (kPrecBits - 1), s1 = s0, s2 = s0, s3 = s0;
    for (int j = 0; j < n; ++j) {
        const uchar4 p = row[j];
        const int kj = k[j];
        s0 += (int)p.x * kj;
        s1 += (int)p.y * kj;
        s2 += (int)p.z * kj;
        s3 += (int)p.w * kj;
    }
    T[((size_t)b * S + y) * RS + u] = make_uchar4(clip_any(s0), clip_any(s1), clip_any(s2), clip_any(s3));
}

__global__ __launch_bounds__(kAgThreads) void augment_geometry_kernel(const unsigned char *__restrict__ packed,
                                                                      const uchar4 *__restrict__ A,
                                                                      const uchar4 *__restrict__ T, uchar4 *__restrict__ G,
                                                                      int S, int RS)
{
    const int b = blockIdx.y;
    const int o = blockIdx.x * kAgThreads + threadIdx.x;
    if (o >= S * S) return;
    const long long *d = sample_desc(packed, b);
    const int y = o / S, x = o - y * S;
    int sx = x, sy = y;
    bool inside = true;
    if (d[kDRot]) {                            // Image.rotate's NEAREST fixed-point map, crop origin folded in
        const long long xx = d[kDRotCoef + 2] + (long long)x * d[kDRotCoef + 0] + (long long)y * d[kDRotCoef + 1];
        const long long yy = d[kDRotCoef + 5] + (long long)x * d[kDRotCoef + 3] + (long long)y * d[kDRotCoef + 4];
        sx = (int)(xx >> 16);
        sy = (int)(yy >> 16);
        inside = sx >= 0 && sx < S && sy >= 0 && sy < S;
    }
    uchar4 v = make_uchar4(0, 0, 0, 0);
    if (inside) {
        if (d[kDMirror]) sx = S - 1 - sx;
        const int R = (int)d[kDR];
        if (R == 0) {
            v = A[((size_t)b * S + sy) * S + sx];
        } else {
            const int off = (int)d[kDOff], u = sx + off, w = sy + off;
            if (u >= 0 && u < R && w >= 0 && w < R) {     // outside: the pad of a shrunk image
                const int *tab = reinterpret_cast<const int *>(d[kDScaleTable]);
                const int taps = (int)d[kDTaps];
                const int ymin = tab[2 * w], n = tab[2 * w + 1];
                const int *k = tab + 2 * (size_t)R + (size_t)w * taps;
                const uchar4 *col = T + ((size_t)b * S + ymin) * RS + u;
                int s0 = 1 << (kPrecBits - 1), s1 = s0, s2 = s0, s3 = s0;
                for (int j = 0; j < n; ++j) {
                    const uchar4 p = col[(size_t)j * RS];
                    const int kj = k[j];
                    s0 += (int)p.x * kj;
                    s1 += (int)p.y * kj;
                    s2 += (int)p.z * kj;
                    s3 += (int)p.w * kj;
                }
                v = make_uchar4(clip_any(s0), clip_any(s1), clip_any(s2), clip_any(s3));
            }
        }
    }
    G[((size_t)b * S + y) * S + x] = v;
}

// ---------------------------------------------------------------------------------------------- (c, d) enhancers, tensors
// Image.blend(degenerate, image, alpha) with alpha a C float: t = fp32(deg + alpha * (px - deg)), clipped, truncated
__device__ __forceinline__ int blend(int deg, int px, float alpha)
{
#pragma clang fp contract(off)
    const float t = (float)deg + alpha * (float)(px - deg);
    return t <= 0.f ? 0 : (t >= 255.f ? 255 : (int)t);
}

// ImageFilter.SMOOTH at an interior pixel, Pillow's ImagingFilter3x3 order: the row below, the row, the row above
__device__ __forceinline__ int smooth(const unsigned char *p, int stride, int c, const float *k)
{
#pragma clang fp contract(off)
    const unsigned char *lo = p + stride, *hi = p - stride;
    float ss = 0.f;
    ss += (float)lo[c - 4] * k[0] + (float)lo[c] * k[1] + (float)lo[c + 4] * k[2];
    ss += (float)p[c - 4] * k[3] + (float)p[c] * k[4] + (float)p[c + 4] * k[5];
    ss += (float)hi[c - 4] * k[6] + (float)hi[c] * k[7] + (float)hi[c + 4] * k[8];
    if (ss <= 0.f) return 0;
    if (ss >= 255.f) return 255;
    return (int)((double)ss + 0.5);
}

__global__ __launch_bounds__(kEnhThreads) void augment_enhance_kernel(const unsigned char *__restrict__ packed,
                                                                      const int *__restrict__ size_table,
                                                                      unsigned char *G, unsigned char *A,
                                                                      float *__restrict__ image, float *__restrict__ label,
                                                                      int S)
{
    __shared__ float lut[4 * 256];
    __shared__ float kern[9];
    __shared__ unsigned long long part[kEnhThreads];
    const float *tl = reinterpret_cast<const float *>(size_table);
    for (int i = threadIdx.x; i < 4 * 256; i += kEnhThreads) lut[i] = tl[kStNorm + i];
    if (threadIdx.x < 9) kern[threadIdx.x] = tl[kStSmooth + threadIdx.x];
    const int b = blockIdx.x;
    const long long *d = sample_desc(packed, b);
    const int n = (int)d[kDEnhCount];
    const int npx = S * S;
    const unsigned char *src = G + (size_t)b * npx * 4;
    unsigned char *dst = A + (size_t)b * npx * 4;
    float *img = image + (size_t)b * 3 * npx, *lab = label + (size_t)b * npx;
    __syncthreads();

    const int passes = n > 0 ? n : 1;          // no enhancer: one pass that only converts
    for (int e = 0; e < passes; ++e) {
        const int op = e < n ? (int)d[kDEnhOp + e] : -1;
        const float alpha = e < n ? __uint_as_float((unsigned)d[kDEnhFactor + e]) : 0.f;
        const bool last = e == passes - 1;
        int mean = 0;
        if (op == TRAMBA_AUG_CONTRAST) {      // ImageStat mean of convert("L"): an exact integer sum, tree-reduced
            unsigned long long s = 0;
            for (int p = threadIdx.x; p < npx; p += kEnhThreads) {
                const unsigned char *q = src + (size_t)p * 4;
                s += (unsigned)((int)q[0] * 19595 + (int)q[1] * 38470 + (int)q[2] * 7471 + 0x8000) >> 16;
            }
            part[threadIdx.x] = s;
            __syncthreads();
            for (int h = kEnhThreads / 2; h > 0; h >>= 1) {
                if ((int)threadIdx.x < h) part[threadIdx.x] += part[threadIdx.x + h];
                __syncthreads();
            }
            mean = (int)((double)part[0] / (double)npx + 0.5);
        }
        for (int p = threadIdx.x; p < npx; p += kEnhThreads) {
            const unsigned char *q = src + (size_t)p * 4;
            int v[4] = {q[0], q[1], q[2], q[3]};
            if (op == TRAMBA_AUG_CONTRAST) {
                for (int c = 0; c < 3; ++c) v[c] = blend(mean, v[c], alpha);
            } else if (op == TRAMBA_AUG_BRIGHTNESS) {
                for (int c = 0; c < 3; ++c) v[c] = blend(0, v[c], alpha);
            } else if (op == TRAMBA_AUG_SHARPNESS) {
                const int y = p / S, x = p - y * S;
                if (x > 0 && x < S - 1 && y > 0 && y < S - 1) {   // the filtered image's edge pixels are copies: blend = px
                    int sm[3];
                    for (int c = 0; c < 3; ++c) sm[c] = smooth(q, S * 4, c, kern);
                    for (int c = 0; c < 3; ++c) v[c] = blend(sm[c], v[c], alpha);
                }
            }
            if (last) {
                for (int c = 0; c < 3; ++c) img[(size_t)c * npx + p] = lut[c * 256 + v[c]];
                lab[p] = lut[768 + v[3]];
            } else {
                *reinterpret_cast<uchar4 *>(dst + (size_t)p * 4) = make_uchar4(v[0], v[1], v[2], v[3]);
            }
        }
        __syncthreads();
        unsigned char *t = const_cast<unsigned char *>(src);
        src = dst;
        dst = t;
    }
}

}  // namespace tramba

using namespace tramba;

extern "C" size_t tramba_augment_source_table_words(int h, int w, int size)
{
    return aug_size_ok(size) && frame_sizes_ok(h, w, size, size) ? source_words(h, w, size) : 0;
}

extern "C" int tramba_augment_source_table(int h, int w, int size, int *table, size_t words)
{
    TRAMBA_CHECK(table, "augment_source_table: null pointer");
    TRAMBA_CHECK(aug_size_ok(size) && frame_sizes_ok(h, w, size, size),
                 "augment_source_table: %dx%d -> %d outside 1 .. %d per source side, 3 .. %d for the output side", h, w,
                 size, TRAMBA_FRAME_MAX_DIM, TRAMBA_FRAME_MAX_OUT);
    TRAMBA_CHECK(words >= source_words(h, w, size), "augment_source_table: %zu words given, %zu needed", words,
                 source_words(h, w, size));
    const double zero[3] = {0, 0, 0}, one[3] = {1, 1, 1};
    const size_t rw = tramba_resize_table_words(h, w, size, size);
    const int rc = tramba_resize_table(h, w, size, size, zero, one, table + 4, rw);
    if (rc != TRAMBA_OK) return rc;
    table[0] = resample_taps(w, size, kFilterBilinear);
    table[1] = resample_taps(h, size, kFilterBilinear);
    table[2] = table[3] = 0;
    nearest_axis(w, size, table + 4 + rw);
    nearest_axis(h, size, table + 4 + rw + size);
    return TRAMBA_OK;
}

extern "C" size_t tramba_augment_size_table_words(int size) { return aug_size_ok(size) ? size_words(size) : 0; }

extern "C" int tramba_augment_size_table(int size, const double *mean, const double *std, int *table, size_t words)
{
#pragma clang fp contract(off)
    TRAMBA_CHECK(table && mean && std, "augment_size_table: null pointer");
    TRAMBA_CHECK(aug_size_ok(size), "augment_size_table: size %d outside 3 .. %d", size, TRAMBA_FRAME_MAX_OUT);
    TRAMBA_CHECK(words >= size_words(size), "augment_size_table: %zu words given, %zu needed", words, size_words(size));
    for (int c = 0; c < 3; ++c) TRAMBA_CHECK(std[c] != 0.0, "augment_size_table: std[%d] is zero", c);
    memset(table, 0, size_words(size) * sizeof(int));
    normalise_lut(mean, std, reinterpret_cast<float *>(table + kStNorm));
    float *mask = reinterpret_cast<float *>(table + kStMask);
    for (int u = 0; u < 256; ++u) mask[u] = (float)u / 255.0f;
    const float smooth_k[9] = {1, 1, 1, 1, 5, 1, 1, 1, 1};
    float *sk = reinterpret_cast<float *>(table + kStSmooth);
    for (int i = 0; i < 9; ++i) sk[i] = smooth_k[i] / 13.0f;
    const int lo = scale_lo(size), hi = scale_hi(size);
    table[kStRange] = lo;
    table[kStRange + 1] = hi;
    size_t at = kStIndex + (size_t)(hi - lo + 1);
    for (int R = lo; R <= hi; ++R) {
        if (R == size) continue;
        const int taps = resample_taps(size, R, kFilterBicubic);
        table[kStIndex + R - lo] = (int)at;
        TRAMBA_CHECK(resample_axis(size, R, kFilterBicubic, taps, table + at, table + at + 2 * (size_t)R),
                     "augment_size_table: tap count out of range");
        at += 2 * (size_t)R + (size_t)R * taps;
    }
    return TRAMBA_OK;
}

extern "C" int tramba_augment_scale_taps(int size, int r)
{
    TRAMBA_CHECK(aug_size_ok(size) && r >= scale_lo(size) && r <= scale_hi(size) && r != size,
                 "augment_scale_taps: R = %d outside %d .. %d for size %d (or the copy R == size)", r,
                 aug_size_ok(size) ? scale_lo(size) : 0, aug_size_ok(size) ? scale_hi(size) : 0, size);
    return resample_taps(size, r, kFilterBicubic);
}

extern "C" int tramba_augment_rotation(int size, int degrees, int *coef)
{
    TRAMBA_CHECK(coef, "augment_rotation: null pointer");
    TRAMBA_CHECK(aug_size_ok(size), "augment_rotation: size %d outside 3 .. %d", size, TRAMBA_FRAME_MAX_OUT);
    TRAMBA_CHECK(rotation_coefficients(size, degrees, coef),
                 "augment_rotation: %d degrees at size %d is not a fixed-point affine rotation", degrees, size);
    return TRAMBA_OK;
}

extern "C" size_t tramba_augment_workspace(int batch, int size)
{
    if (batch < 1 || batch > 65535 || !aug_size_ok(size)) return 0;
    return (size_t)batch * size * 4 * (2 * (size_t)size + scale_hi(size));
}

extern "C" int tramba_augment_batch(const unsigned char *packed, const int64_t *desc_host, size_t packed_bytes,
                                    const int *size_table, float *image, float *label, void *workspace,
                                    size_t workspace_bytes, int batch, int size, void *stream)
{
    TRAMBA_CHECK(packed && desc_host && size_table && image && label && workspace, "augment_batch: null pointer");
    TRAMBA_CHECK(batch >= 1 && batch <= 65535, "augment_batch: batch %d outside 1 .. 65535", batch);
    TRAMBA_CHECK(aug_size_ok(size), "augment_batch: size %d outside 3 .. %d", size, TRAMBA_FRAME_MAX_OUT);
    TRAMBA_CHECK(workspace_bytes >= tramba_augment_workspace(batch, size), "augment_batch: workspace %zu bytes, %zu needed",
                 workspace_bytes, tramba_augment_workspace(batch, size));
    const size_t head = (size_t)batch * TRAMBA_AUG_DESC_WORDS * 8;
    TRAMBA_CHECK(packed_bytes >= head, "augment_batch: %zu packed bytes hold no %d descriptors", packed_bytes, batch);
    const int lo = scale_lo(size), hi = scale_hi(size);
    for (int b = 0; b < batch; ++b) {
        const int64_t *d = desc_host + (size_t)b * TRAMBA_AUG_DESC_WORDS;
        const int64_t h = d[kDH], w = d[kDW], R = d[kDR];
        TRAMBA_CHECK(h >= 1 && w >= 1 && h <= TRAMBA_FRAME_MAX_DIM && w <= TRAMBA_FRAME_MAX_DIM,
                     "augment_batch: sample %d is %lldx%lld, outside 1 .. %d per side", b, (long long)h, (long long)w,
                     TRAMBA_FRAME_MAX_DIM);
        TRAMBA_CHECK(d[kDImg] >= (int64_t)head && d[kDMask] >= (int64_t)head &&
                         (uint64_t)d[kDImg] + (uint64_t)(h * w * 3) <= packed_bytes &&
                         (uint64_t)d[kDMask] + (uint64_t)(h * w) <= packed_bytes,
                     "augment_batch: sample %d lies outside the %zu packed bytes", b, packed_bytes);
        TRAMBA_CHECK(d[kDSrcTable] != 0, "augment_batch: sample %d has no source table", b);
        TRAMBA_CHECK(R == 0 || (R >= lo && R <= hi && R != size && d[kDScaleTable] != 0 &&
                                d[kDTaps] == resample_taps(size, (int)R, kFilterBicubic) &&
                                d[kDOff] == (R - size - ((R - size) & 1)) / 2),
                     "augment_batch: sample %d: scale R = %lld outside %d .. %d or inconsistent", b, (long long)R, lo, hi);
        TRAMBA_CHECK((d[kDMirror] | 1) == 1 && (d[kDRot] | 1) == 1, "augment_batch: sample %d: bad flip / rotate flags", b);
        TRAMBA_CHECK(d[kDEnhCount] >= 0 && d[kDEnhCount] <= 3, "augment_batch: sample %d: %lld enhancers", b,
                     (long long)d[kDEnhCount]);
        for (int e = 0; e < (int)d[kDEnhCount]; ++e)
            TRAMBA_CHECK(d[kDEnhOp + e] >= TRAMBA_AUG_CONTRAST && d[kDEnhOp + e] <= TRAMBA_AUG_SHARPNESS,
                         "augment_batch: sample %d: enhancer %lld unknown", b, (long long)d[kDEnhOp + e]);
    }
    const int RS = hi;
    unsigned char *A = static_cast<unsigned char *>(workspace);
    unsigned char *T = A + (size_t)batch * size * size * 4;
    unsigned char *G = T + (size_t)batch * size * RS * 4;
    hipStream_t s = (hipStream_t)stream;

    const int slab_max = kAgThreads * kAgMaxAcc / 3, nslab = (size + slab_max - 1) / slab_max;
    const int slab = (size + nslab - 1) / nslab;
    const int band_max = kAgThreads * kAgMaxAcc / (3 * slab);
    int band = (int)((long long)size * nslab * batch / kAgWantBlocks);
    band = band < 1 ? 1 : (band > band_max ? band_max : band);
    const int chunk = kAgLdsBytes / (3 * slab);
    hipLaunchKernelGGL(augment_resize_kernel, dim3(nslab, (size + band - 1) / band, batch), dim3(kAgThreads),
                       (size_t)chunk * 3 * slab, s, packed, A, size, slab, band, chunk);
    TRAMBA_LAUNCH_CHECK();
    hipLaunchKernelGGL(augment_scale_rows_kernel, dim3((unsigned)(((size_t)size * RS + kAgThreads - 1) / kAgThreads), batch),
                       dim3(kAgThreads), 0, s, packed, reinterpret_cast<const uchar4 *>(A), reinterpret_cast<uchar4 *>(T),
                       size, RS);
    TRAMBA_LAUNCH_CHECK();
    hipLaunchKernelGGL(augment_geometry_kernel, dim3((unsigned)(((size_t)size * size + kAgThreads - 1) / kAgThreads), batch),
                       dim3(kAgThreads), 0, s, packed, reinterpret_cast<const uchar4 *>(A),
                       reinterpret_cast<const uchar4 *>(T), reinterpret_cast<uchar4 *>(G), size, RS);
    TRAMBA_LAUNCH_CHECK();
    hipLaunchKernelGGL(augment_enhance_kernel, dim3(batch), dim3(kEnhThreads), 0, s, packed, size_table, G, A, image, label,
                       size);
    TRAMBA_LAUNCH_CHECK();
    return TRAMBA_OK;
}
