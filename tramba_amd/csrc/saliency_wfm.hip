// The weighted F-measure of Evaluation/metrics.py:379-441 on the GPU: an exact Euclidean feature transform of the masks
// (scipy.ndimage.distance_transform_edt(~gt, return_indices=True), index for index, ties included) and the fused sums
// behind R, P and Q.
//
// Feature transform: Maurer's separable algorithm as scipy's _ComputeFT / _VoronoiFT run it on a 2-D image.
//   pass 1 (ft_columns_kernel, one thread per column segment): every pixel takes the nearest mask row of its own
//     column, the smaller row on a tie.  The row is kept in `idx` until pass 2.
//   pass 2 (ft_rows_kernel, one wave per image row): the columns with a pass-1 feature are the sites; their lower
//     envelope is built on a stack in LDS (pop while c vR - b uR - a wR - a b c > 0), then walked left to right with
//     a pointer that advances only while the next site is STRICTLY closer.  Both steps are sequential per row and run
//     on lane 0; the other lanes stage the row in and the result out.  All arithmetic is in integers (int64 where the
//     envelope products reach ~1e11), so every decision equals scipy's exact fp64 one.
// Weighted-F sums: per-chunk min / max of pred (wfm_minmax_kernel); per 16 x 64 tile (wfm_tile_kernel) the spread error
//   Et = |p(nearest mask pixel) - 1| is staged with a 3-pixel zero halo in LDS, filtered by the 7x7 Gaussian in fp64
//   (stored fp32, as scipy does for an fp32 input), and MIN_E_EA, the pixel weight and Ew are summed per tile in fp64;
//   wfm_finish_kernel adds the tiles of an image in a fixed order.  No atomics: bitwise reproducible, and an image's sums
//   do not depend on the batch it is in.
#include "common.h"

namespace tramba {

constexpr int kFtCols = 64, kFtSegs = 16;
constexpr int kMmThreads = 256, kMmChunk = 8192;
constexpr int kTileH = 16, kTileW = 64, kTileThreads = 256, kTileRows = kTileH / (kTileThreads / kTileW);
constexpr int kHaloH = kTileH + 6, kHaloW = kTileW + 6;
constexpr int kFinThreads = 256;

struct Gauss7 {
    double w[49];
};

// ---------------------------------------------------------------------------------------------- feature transform
__global__ __launch_bounds__(kFtCols * kFtSegs) void ft_columns_kernel(const unsigned char *__restrict__ gt,
                                                                        int *__restrict__ f, int H, int W)
{
    // a block takes kFtCols columns, each cut into kFtSegs row segments (one thread each): the segments' first / last
    // mask rows meet in LDS, so every thread knows the nearest mask row above and below its segment
    __shared__ int seg_first[kFtSegs][kFtCols], seg_last[kFtSegs][kFtCols];
    const int cx = threadIdx.x % kFtCols, sg = threadIdx.x / kFtCols;
    const int c = blockIdx.x * kFtCols + cx;
    const int len = (H + kFtSegs - 1) / kFtSegs, r_begin = min(H, sg * len), r_end = min(H, r_begin + len);
    const bool on = c < W;
    const size_t base = (size_t)blockIdx.y * H * W + (on ? c : 0);
    const unsigned char *g = gt + base;
    int *o = f + base;
    int first = -1, last = -1;
    if (on) {
#pragma unroll 8
        for (int r = r_begin; r < r_end; ++r) {
            if (g[(size_t)r * W]) {
                first = first < 0 ? r : first;
                last = r;
            }
        }
    }
    seg_first[sg][cx] = first;
    seg_last[sg][cx] = last;
    __syncthreads();
    if (!on) return;
    int prev = -1, next = -1;
    for (int t = sg - 1; t >= 0 && prev < 0; --t) prev = seg_last[t][cx];
    for (int t = sg + 1; t < kFtSegs && next < 0; ++t) next = seg_first[t][cx];
#pragma unroll 8
    for (int r = r_begin; r < r_end; ++r) {
        if (g[(size_t)r * W]) prev = r;
        o[(size_t)r * W] = prev;
    }
#pragma unroll 8
    for (int r = r_end - 1; r >= r_begin; --r) {
        if (g[(size_t)r * W]) next = r;
        const int up = o[(size_t)r * W];
        o[(size_t)r * W] = up < 0 || (next >= 0 && next - r < r - up) ? next : up;
    }
}

// site of the envelope, packed: row << 16 | column (H, W <= TRAMBA_WFM_MAX_DIM <= 32768)
__device__ __forceinline__ int site_pack(int r, int c) { return (r << 16) | c; }

__global__ __launch_bounds__(kWave) void ft_rows_kernel(int *__restrict__ f, int *__restrict__ dist2, int H, int W)
{
    extern __shared__ int ft_lds[];
    const int wp = (W + 3) & ~3;
    int *row = ft_lds, *stk = ft_lds + wp;   // row: pass-1 rows (-1: no site) -> final packed sites; stk: the envelope
    const int i = blockIdx.x, lane = threadIdx.x;
    const size_t base = ((size_t)blockIdx.y * H + i) * W;
    for (int j = lane; j < wp; j += kWave) row[j] = j < W ? f[base + j] : -1;
    __syncthreads();
    if (lane == 0) {
        // ---- lower envelope; the two top sites live in registers, the rest of the stack in LDS
        int top = -1, s0c = 0, s0r = 0, s1c = 0, s1r = 0;
        for (int j0 = 0; j0 < wp; j0 += 4) {
            const int4 q = *reinterpret_cast<const int4 *>(row + j0);
            const int rr[4] = {q.x, q.y, q.z, q.w};
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const int r = rr[k], j = j0 + k;
                if (r < 0) continue;
                const long long wR = (long long)(r - i) * (r - i);
                while (top >= 1) {
                    const long long a = s1c - s0c, b = j - s1c, c = a + b;
                    const long long uR = (long long)(s0r - i) * (s0r - i), vR = (long long)(s1r - i) * (s1r - i);
                    if (c * vR - b * uR - a * wR - a * b * c <= 0) break;
                    --top;
                    s1c = s0c;
                    s1r = s0r;
                    if (top >= 1) {
                        const int s = stk[top - 1];
                        s0r = s >> 16;
                        s0c = s & 0xffff;
                    }
                }
                stk[++top] = site_pack(r, j);
                s0c = s1c;
                s0r = s1r;
                s1c = j;
                s1r = r;
            }
        }
        // ---- walk: column j takes the first site from the pointer on that is not beaten strictly by the next one
        if (top < 0) {
            for (int j = 0; j < W; ++j) row[j] = -1;   // empty mask: no feature anywhere
        } else {
            int l = 0, cs = stk[0], ns = top >= 1 ? stk[1] : 0;
            for (int j = 0; j < W; ++j) {
                int dr = (cs >> 16) - i, dc = (cs & 0xffff) - j;
                int d1 = dr * dr + dc * dc;
                while (l < top) {
                    dr = (ns >> 16) - i;
                    dc = (ns & 0xffff) - j;
                    const int d2 = dr * dr + dc * dc;
                    if (d1 <= d2) break;
                    d1 = d2;
                    cs = ns;
                    ++l;
                    if (l < top) ns = stk[l + 1];
                }
                row[j] = cs;
            }
        }
    }
    __syncthreads();
    for (int j = lane; j < W; j += kWave) {
        const int s = row[j];
        if (s < 0) {
            f[base + j] = -1;
            dist2[base + j] = -1;
        } else {
            const int r = s >> 16, c = s & 0xffff, dr = r - i, dc = c - j;
            f[base + j] = r * W + c;
            dist2[base + j] = dr * dr + dc * dc;
        }
    }
}

// ---------------------------------------------------------------------------------------------- weighted-F sums
__global__ __launch_bounds__(kMmThreads) void wfm_minmax_kernel(const float *__restrict__ pred, float *__restrict__ mm,
                                                                int n, int nchunk)
{
    __shared__ float red[2 * (kMmThreads / kWave)];
    const int img = blockIdx.y, k = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const float *p = pred + (size_t)img * n;
    const int end = min(n, (k + 1) * kMmChunk);
    float mn = INFINITY, mx = -INFINITY;
    for (int q = k * kMmChunk + tid; q < end; q += kMmThreads) {
        const float v = p[q];
        mn = fminf(mn, v);
        mx = fmaxf(mx, v);
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        mn = fminf(mn, __shfl_xor(mn, o, 64));
        mx = fmaxf(mx, __shfl_xor(mx, o, 64));
    }
    if (lane == 0) {
        red[wave] = mn;
        red[kMmThreads / kWave + wave] = mx;
    }
    __syncthreads();
    if (tid == 0) {
        for (int w = 1; w < kMmThreads / kWave; ++w) {
            mn = fminf(mn, red[w]);
            mx = fmaxf(mx, red[kMmThreads / kWave + w]);
        }
        mm[((size_t)img * nchunk + k) * 2 + 0] = mn;
        mm[((size_t)img * nchunk + k) * 2 + 1] = mx;
    }
}

__device__ __forceinline__ double wave_sum_d(double v)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

__global__ __launch_bounds__(kTileThreads) void wfm_tile_kernel(const float *__restrict__ pred,
                                                                const unsigned char *__restrict__ gt,
                                                                const int *__restrict__ idx, const int *__restrict__ dist2,
                                                                const float *__restrict__ mm, Gauss7 gw,
                                                                double *__restrict__ part, int H, int W, int nchunk)
{
#pragma clang fp contract(off)   // scipy's correlate and numpy multiply and add separately
    __shared__ float et[kHaloH * kHaloW];
    __shared__ float red_f[2 * (kTileThreads / kWave)];
    __shared__ double red_d[3 * (kTileThreads / kWave)];
    const int img = blockIdx.z, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int ntiles = gridDim.x * gridDim.y, tile = blockIdx.y * gridDim.x + blockIdx.x;
    const int y0 = blockIdx.y * kTileH, x0 = blockIdx.x * kTileW;
    const size_t n = (size_t)H * W, ib = (size_t)img * n;
    double *out = part + ((size_t)img * ntiles + tile) * 3;
    // an empty mask has no feature anywhere (idx = -1): nothing to gather; the host reports wfm = 0
    if (idx[ib] < 0) {
        if (tid < 3) out[tid] = 0.0;
        return;
    }
    // min / max of the image from the chunk partials (exact in any order)
    float mn = INFINITY, mx = -INFINITY;
    for (int k = tid; k < nchunk; k += kTileThreads) {
        mn = fminf(mn, mm[((size_t)img * nchunk + k) * 2 + 0]);
        mx = fmaxf(mx, mm[((size_t)img * nchunk + k) * 2 + 1]);
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        mn = fminf(mn, __shfl_xor(mn, o, 64));
        mx = fmaxf(mx, __shfl_xor(mx, o, 64));
    }
    if (lane == 0) {
        red_f[wave] = mn;
        red_f[kTileThreads / kWave + wave] = mx;
    }
    __syncthreads();
    for (int w = 0; w < kTileThreads / kWave; ++w) {
        mn = fminf(mn, red_f[w]);
        mx = fmaxf(mx, red_f[kTileThreads / kWave + w]);
    }
    const bool norm = mx != mn;
    const float span = mx - mn;
    const float *p = pred + ib;

    // Et over the tile and its halo: the error of the nearest mask pixel (a mask pixel is its own nearest), 0 outside
    for (int q = tid; q < kHaloH * kHaloW; q += kTileThreads) {
        const int r = y0 - 3 + q / kHaloW, c = x0 - 3 + q % kHaloW;
        float e = 0.0f;
        if (r >= 0 && r < H && c >= 0 && c < W) {
            float v = p[idx[ib + (size_t)r * W + c]];
            if (norm) v = (v - mn) / span;
            e = fabsf(v - 1.0f);
        }
        et[q] = e;
    }
    __syncthreads();

    const int tx = tid % kTileW, ty = (tid / kTileW) * kTileRows;
    const double k_ln = -0.6931471805599453 / 5.0;    // np.log(0.5) / 5
    double s_fg = 0.0, s_bg = 0.0, cnt = 0.0;
    const int c = x0 + tx;
#pragma unroll
    for (int k = 0; k < kTileRows; ++k) {
        const int r = y0 + ty + k;
        if (r >= H || c >= W) continue;
        const size_t o = ib + (size_t)r * W + c;
        float v = pred[o];
        if (norm) v = (v - mn) / span;
        if (gt[o]) {
            double acc = 0.0;
            const float *t = et + (ty + k) * kHaloW + tx;
#pragma unroll
            for (int dy = 0; dy < 7; ++dy)
#pragma unroll
                for (int dx = 0; dx < 7; ++dx) acc += (double)t[dy * kHaloW + dx] * gw.w[dy * 7 + dx];
            const float ea = (float)acc, e = fabsf(v - 1.0f);
            s_fg += (double)(ea < e ? ea : e);
            cnt += 1.0;
        } else {
            const double b = 2.0 - exp(k_ln * sqrt((double)dist2[o]));
            s_bg += (double)fabsf(v) * b;
        }
    }
    // fixed-order block sum
    s_fg = wave_sum_d(s_fg);
    s_bg = wave_sum_d(s_bg);
    cnt = wave_sum_d(cnt);
    if (lane == 0) {
        red_d[wave * 3 + 0] = cnt;
        red_d[wave * 3 + 1] = s_fg;
        red_d[wave * 3 + 2] = s_bg;
    }
    __syncthreads();
    if (tid < 3) {
        double s = 0.0;
        for (int w = 0; w < kTileThreads / kWave; ++w) s += red_d[w * 3 + tid];
        out[tid] = s;
    }
}

__global__ __launch_bounds__(kFinThreads) void wfm_finish_kernel(const double *__restrict__ part, double *__restrict__ sums,
                                                                 int ntiles)
{
    __shared__ double red[3 * (kFinThreads / kWave)];
    const int img = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const double *pp = part + (size_t)img * ntiles * 3;
    double s[3] = {0.0, 0.0, 0.0};
    for (int t = tid; t < ntiles; t += kFinThreads) {
        s[0] += pp[t * 3 + 0];
        s[1] += pp[t * 3 + 1];
        s[2] += pp[t * 3 + 2];
    }
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        s[k] = wave_sum_d(s[k]);
        if (lane == 0) red[wave * 3 + k] = s[k];
    }
    __syncthreads();
    if (tid < 3) {
        double v = 0.0;
        for (int w = 0; w < kFinThreads / kWave; ++w) v += red[w * 3 + tid];
        sums[(size_t)img * 3 + tid] = v;
    }
}

struct WfmLayout {
    int nchunk, tx, ty;
    size_t mm_bytes, part_off, bytes;
};

static WfmLayout wfm_layout(int batch, int h, int w)
{
    WfmLayout L;
    const long n = (long)h * w;
    L.nchunk = (int)((n + kMmChunk - 1) / kMmChunk);
    L.tx = (w + kTileW - 1) / kTileW;
    L.ty = (h + kTileH - 1) / kTileH;
    L.mm_bytes = (size_t)batch * L.nchunk * 2 * sizeof(float);
    L.part_off = (L.mm_bytes + 255) & ~(size_t)255;
    L.bytes = L.part_off + (size_t)batch * L.tx * L.ty * 3 * sizeof(double);
    return L;
}

static bool wfm_shape_ok(int batch, int h, int w)
{
    return batch > 0 && h > 0 && w > 0 && h <= TRAMBA_WFM_MAX_DIM && w <= TRAMBA_WFM_MAX_DIM && batch <= 65535;
}

}  // namespace tramba

using namespace tramba;

extern "C" int tramba_feature_transform(const unsigned char *gt, int *idx, int *dist2, int batch, int h, int w, void *stream)
{
    TRAMBA_CHECK(gt && idx && dist2, "feature_transform: null tensor");
    TRAMBA_CHECK(wfm_shape_ok(batch, h, w), "feature_transform: shape (%d, %d, %d) outside 1 .. %d per side", batch, h, w,
                 TRAMBA_WFM_MAX_DIM);
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(ft_columns_kernel, dim3((w + kFtCols - 1) / kFtCols, batch), dim3(kFtCols * kFtSegs), 0, s, gt, idx,
                       h, w);
    TRAMBA_LAUNCH_CHECK();
    const size_t lds = 2 * (size_t)((w + 3) & ~3) * sizeof(int);
    hipLaunchKernelGGL(ft_rows_kernel, dim3(h, batch), dim3(kWave), lds, s, idx, dist2, h, w);
    TRAMBA_LAUNCH_CHECK();
    return TRAMBA_OK;
}

extern "C" size_t tramba_weighted_f_workspace(int batch, int h, int w)
{
    return wfm_shape_ok(batch, h, w) ? wfm_layout(batch, h, w).bytes : 0;
}

extern "C" int tramba_weighted_f_sums(const float *pred, const unsigned char *gt, const int *idx, const int *dist2,
                                      const double *gauss, double *sums, void *workspace, size_t workspace_bytes, int batch,
                                      int h, int w, void *stream)
{
    TRAMBA_CHECK(pred && gt && idx && dist2 && gauss && sums && workspace, "weighted_f_sums: null pointer");
    TRAMBA_CHECK(wfm_shape_ok(batch, h, w), "weighted_f_sums: shape (%d, %d, %d) outside 1 .. %d per side", batch, h, w,
                 TRAMBA_WFM_MAX_DIM);
    const WfmLayout L = wfm_layout(batch, h, w);
    TRAMBA_CHECK(workspace_bytes >= L.bytes, "weighted_f_sums: workspace of %zu bytes, %zu needed", workspace_bytes, L.bytes);
    Gauss7 gw;
    for (int k = 0; k < 49; ++k) gw.w[k] = gauss[k];
    float *mm = reinterpret_cast<float *>(workspace);
    double *part = reinterpret_cast<double *>(reinterpret_cast<char *>(workspace) + L.part_off);
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(wfm_minmax_kernel, dim3(L.nchunk, batch), dim3(kMmThreads), 0, s, pred, mm, h * w, L.nchunk);
    TRAMBA_LAUNCH_CHECK();
    hipLaunchKernelGGL(wfm_tile_kernel, dim3(L.tx, L.ty, batch), dim3(kTileThreads), 0, s, pred, gt, idx, dist2, mm, gw,
                       part, h, w, L.nchunk);
    TRAMBA_LAUNCH_CHECK();
    hipLaunchKernelGGL(wfm_finish_kernel, dim3(batch), dim3(kFinThreads), 0, s, part, sums, L.tx * L.ty);
    TRAMBA_LAUNCH_CHECK();
    return TRAMBA_OK;
}
