// Fused element kernels of the TRAINING path (round 3): what used to be chains of small framework launches between the
// library's GEMM / scan / stencil kernels of a step -- residual adds, stochastic-depth multiplies, activation forwards and
// their gradients, gathers, zero fills, casts -- folded into the neighbouring passes.  All HBM-bound row kernels.
//
//   add_layernorm      x' = x + y * mask[sample]  (residual + stochastic depth, vmamba.py:384-396)  and  n = LayerNorm(x'),
//                      optionally also act(n): ONE pass where autograd issued addcmul -> layer_norm -> gelu.
//   ss2d_bwd_prep      after the scan backward: the dt-rank rows of x_dbl gathered into sequence order (the operand of the
//                      dt_projs_weight gradient) and the per-channel-tile partial sums of dB / dC added up in a fixed order
//                      (the scan backward writes partials instead of fp32 atomics: reproducible).
//   ss2d_bwd_assemble  the x_dbl-row gradients from sequence order back to spatial order through the inverse table (a gather-
//                      sum: deterministic also for the many-to-one Helix lines, no zero fill, no index_add_), cast to the
//                      activation dtype the x_proj gradient GEMMs read.
//   dw_unpack_grad     gradient of the folded 7x7 multi-scale stencil (tramba_dw_pack) handed back to the 3x3 / 5x5 / 7x7
//                      parameters in their own (C, 1, ks, ks) layouts; single stencils: tap-major -> (C, 1, ks, ks).
#include <stdlib.h>
#include <string.h>

#include "common.h"
#include "norm.h"

namespace tramba {

// ------------------------------------------------------------------------------------------------ add + LayerNorm
// rows form: LPR lanes per row (C <= 64 * V), 64 / LPR rows per wave.
// GATE (both forms): nact = act(n) * silu(gate[row, :]) -- SS2D's z gate (vmamba.py:288-290) in the dual store; gate (rows, C) T
// holds the pre-activation.  Statistics, the masked add and n do not see it.
template <typename T, int V, int LPR, bool GATE>
__device__ __forceinline__ void add_ln_rows_body(const T *__restrict__ x, const T *__restrict__ yadd,
                                                 const float *__restrict__ mask, long rps, const float *__restrict__ w,
                                                 const float *__restrict__ bvec, T *__restrict__ xsum, T *__restrict__ n,
                                                 T *__restrict__ nact, long rows, int C, float eps, int act,
                                                 const T *__restrict__ gate)
{
    const RowLane<V, LPR> ln;
    const long row = ln.row();
    const bool rok = row < rows;
    const int c0 = ln.c0();
    const bool cok = ln.cok(C);
    float v[V];
#pragma unroll
    for (int i = 0; i < V; ++i) v[i] = 0.f;
    if (rok && cok) {
        load_pack<T, V>(x + row * C + c0, v);
        if (yadd) {
            float yv[V];
            load_pack<T, V>(yadd + row * C + c0, yv);
            const float m = mask ? mask[row / rps] : 1.f;
            // the sum is what the next layers (and the backward's recomputed statistics) read: round it to T first
#pragma unroll
            for (int i = 0; i < V; ++i) v[i] = Cvt<T>::to_f(Cvt<T>::from_f(fmaf(yv[i], m, v[i])));
            store_pack<T, V>(xsum + row * C + c0, v);
        }
    }
    float s = 0.f;
#pragma unroll
    for (int i = 0; i < V; ++i) s += v[i];
    const float mean = sub_sum<LPR>(s) / (float)C;
    float q = 0.f;
#pragma unroll
    for (int i = 0; i < V; ++i) {
        const float t = cok ? v[i] - mean : 0.f;
        q = fmaf(t, t, q);
    }
    const float rstd = rsqrtf(sub_sum<LPR>(q) / (float)C + eps);
    if (!(rok && cok)) return;
    float wv[V], bv[V], o[V];
    load_pack<float, V>(w + c0, wv);
    load_pack<float, V>(bvec + c0, bv);
#pragma unroll
    for (int i = 0; i < V; ++i) o[i] = (v[i] - mean) * rstd * wv[i] + bv[i];
    store_pack<T, V>(n + row * C + c0, o);
    if (nact) {
        // the activation of the value AS STORED (the consumer's backward differentiates at the stored pre-activation)
#pragma unroll
        for (int i = 0; i < V; ++i) o[i] = apply_act(Cvt<T>::to_f(Cvt<T>::from_f(o[i])), act);
        if constexpr (GATE) {
            float zv[V];
            load_pack<T, V>(gate + row * C + c0, zv);
#pragma unroll
            for (int i = 0; i < V; ++i) o[i] *= siluf_(zv[i]);
        }
        store_pack<T, V>(nact + row * C + c0, o);
    }
}

template <typename T, int V, int LPR>
__global__ __launch_bounds__(256) void add_ln_rows_kernel(const T *__restrict__ x, const T *__restrict__ yadd,
                                                         const float *__restrict__ mask, long rps,
                                                         const float *__restrict__ w, const float *__restrict__ bvec,
                                                         T *__restrict__ xsum, T *__restrict__ n, T *__restrict__ nact,
                                                         long rows, int C, float eps, int act)
{
    add_ln_rows_body<T, V, LPR, false>(x, yadd, mask, rps, w, bvec, xsum, n, nact, rows, C, eps, act, nullptr);
}

template <typename T, int V, int LPR>
__global__ __launch_bounds__(256) void add_ln_rows_gate_kernel(const T *__restrict__ x, const T *__restrict__ yadd,
                                                              const float *__restrict__ mask, long rps,
                                                              const float *__restrict__ w, const float *__restrict__ bvec,
                                                              T *__restrict__ xsum, T *__restrict__ n,
                                                              T *__restrict__ nact, long rows, int C, float eps, int act,
                                                              const T *__restrict__ gate)
{
    add_ln_rows_body<T, V, LPR, true>(x, yadd, mask, rps, w, bvec, xsum, n, nact, rows, C, eps, act, gate);
}

// wave form: one wave per row, NIT = ceil(C / (64 V)) iterations.
template <typename T, int V, bool GATE>
__device__ __forceinline__ void add_ln_wave_body(const T *__restrict__ x, const T *__restrict__ yadd,
                                                 const float *__restrict__ mask, long rps, const float *__restrict__ w,
                                                 const float *__restrict__ bvec, T *__restrict__ xsum, T *__restrict__ n,
                                                 T *__restrict__ nact, long rows, int C, float eps, int act,
                                                 const T *__restrict__ gate)
{
    const int lane = threadIdx.x & (kWave - 1);
    const long row = (long)blockIdx.x * (blockDim.x >> 6) + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    if (row >= rows) return;
    const int nit = (C + kWave * V - 1) / (kWave * V);
    float acc[kNormMaxIt][V];
    const float m = (yadd && mask) ? mask[row / rps] : 1.f;
#pragma unroll
    for (int it = 0; it < kNormMaxIt; ++it) {
#pragma unroll
        for (int v = 0; v < V; ++v) acc[it][v] = 0.f;
        if (it < nit) {
            const int c0 = (it * kWave + lane) * V;
            if (c0 + V <= C) {
                load_pack<T, V>(x + row * C + c0, acc[it]);
                if (yadd) {
                    float yv[V];
                    load_pack<T, V>(yadd + row * C + c0, yv);
#pragma unroll
                    for (int v = 0; v < V; ++v) acc[it][v] = Cvt<T>::to_f(Cvt<T>::from_f(fmaf(yv[v], m, acc[it][v])));
                    store_pack<T, V>(xsum + row * C + c0, acc[it]);
                }
            }
        }
    }
    float mean, rstd;
    wave_layernorm<V>(acc, nit, C, lane, eps, mean, rstd);
#pragma unroll
    for (int it = 0; it < kNormMaxIt; ++it) {
        if (it < nit) {
            const int c0 = (it * kWave + lane) * V;
            if (c0 + V <= C) {
                float o[V];
#pragma unroll
                for (int v = 0; v < V; ++v) o[v] = (acc[it][v] - mean) * rstd * w[c0 + v] + bvec[c0 + v];
                store_pack<T, V>(n + row * C + c0, o);
                if (nact) {
#pragma unroll
                    for (int v = 0; v < V; ++v) o[v] = apply_act(Cvt<T>::to_f(Cvt<T>::from_f(o[v])), act);
                    if constexpr (GATE) {
                        float zv[V];
                        load_pack<T, V>(gate + row * C + c0, zv);
#pragma unroll
                        for (int v = 0; v < V; ++v) o[v] *= siluf_(zv[v]);
                    }
                    store_pack<T, V>(nact + row * C + c0, o);
                }
            }
        }
    }
}

template <typename T, int V>
__global__ __launch_bounds__(256) void add_ln_wave_kernel(const T *__restrict__ x, const T *__restrict__ yadd,
                                                         const float *__restrict__ mask, long rps,
                                                         const float *__restrict__ w, const float *__restrict__ bvec,
                                                         T *__restrict__ xsum, T *__restrict__ n, T *__restrict__ nact,
                                                         long rows, int C, float eps, int act)
{
    add_ln_wave_body<T, V, false>(x, yadd, mask, rps, w, bvec, xsum, n, nact, rows, C, eps, act, nullptr);
}

template <typename T, int V>
__global__ __launch_bounds__(256) void add_ln_wave_gate_kernel(const T *__restrict__ x, const T *__restrict__ yadd,
                                                              const float *__restrict__ mask, long rps,
                                                              const float *__restrict__ w, const float *__restrict__ bvec,
                                                              T *__restrict__ xsum, T *__restrict__ n,
                                                              T *__restrict__ nact, long rows, int C, float eps, int act,
                                                              const T *__restrict__ gate)
{
    add_ln_wave_body<T, V, true>(x, yadd, mask, rps, w, bvec, xsum, n, nact, rows, C, eps, act, gate);
}

template <typename T>
static int launch_add_ln(const void *x, const void *y, const float *mask, long rps, const float *w, const float *b,
                         void *xsum, void *n, void *nact, long rows, int c, int dtype, float eps, int act, hipStream_t s,
                         const void *gate = nullptr)
{
    const RowForm f = row_form(c, dtype);
    const dim3 block(256);
    if (f.ok && aligned16(w) && aligned16(b)) {   // (unaligned parameters: the wave form reads them element by element)
        const dim3 grid((unsigned)rows_grid(rows_waves(rows, f.lpr)));
        with_lpr(f.lpr, [&](auto L) {
            constexpr int LPR = decltype(L)::value;
            if (gate)
                hipLaunchKernelGGL((add_ln_rows_gate_kernel<T, kRowVec<T>, LPR>), grid, block, 0, s, (const T *)x, (const T *)y,
                                   mask, rps, w, b, (T *)xsum, (T *)n, (T *)nact, rows, c, eps, act, (const T *)gate);
            else
                hipLaunchKernelGGL((add_ln_rows_kernel<T, kRowVec<T>, LPR>), grid, block, 0, s, (const T *)x, (const T *)y, mask,
                                   rps, w, b, (T *)xsum, (T *)n, (T *)nact, rows, c, eps, act);
        });
        TRAMBA_LAUNCH_CHECK();
        return TRAMBA_OK;
    }
    const int v = norm_vec(c, f.vm);
    if ((c + kWave * v - 1) / (kWave * v) > kNormMaxIt) {
        set_error("add_layernorm: C=%d too large", c);
        return TRAMBA_ERR_UNSUPPORTED;
    }
    const dim3 grid((unsigned)rows_grid(rows));
    with_norm_vec<T>(v, [&](auto Vc) {
        constexpr int V = decltype(Vc)::value;
        if (gate)
            hipLaunchKernelGGL((add_ln_wave_gate_kernel<T, V>), grid, block, 0, s, (const T *)x, (const T *)y, mask, rps, w, b,
                               (T *)xsum, (T *)n, (T *)nact, rows, c, eps, act, (const T *)gate);
        else
            hipLaunchKernelGGL((add_ln_wave_kernel<T, V>), grid, block, 0, s, (const T *)x, (const T *)y, mask, rps, w, b,
                               (T *)xsum, (T *)n, (T *)nact, rows, c, eps, act);
    });
    TRAMBA_LAUNCH_CHECK();
    return TRAMBA_OK;
}

// ------------------------------------------------------------------------------------------------ SS2D backward glue
// thread = one (b, k, i) sequence position; R8 = padded rank count, N = d_state, BC = (2N + 3) & ~3, RG = R8 + BC (N = 1:
// RG = R8 + 4).
//   ranks  (B, K, L, R8) T     = xdbl[b, table[k][i], k*RG + 0 .. R8)          (the dt-rank rows in sequence order)
//   g_seq  (B, K, L, RG) f32   columns R8 + n / R8 + N + n = sum over the CT channel tiles of the scan backward's dB_n / dC_n
//                              partials (bpart / cpart: (B, K, CT, N, L) f32), the remaining pad columns = 0; the rank columns
//                              are written by tramba_rows_gemm_cl afterwards
template <typename T>
__global__ __launch_bounds__(256) void ss2d_bwd_prep_kernel(const float *__restrict__ xdbl, const int32_t *__restrict__ table,
                                                           const float *__restrict__ bpart, const float *__restrict__ cpart,
                                                           T *__restrict__ ranks, float *__restrict__ gseq, int L, int K,
                                                           int R8, int CT, int N, int BC)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= L) return;
    const int k = blockIdx.y, b = blockIdx.z;
    const int RG = R8 + BC, PC = K * RG;
    const int p = table[(long)k * L + i];
    const float *src = xdbl + ((long)b * L + p) * PC + (long)k * RG;
    T *dst = ranks + (((long)b * K + k) * L + i) * R8;
    for (int j = 0; j < R8; j += 4) {
        const float4 v = *reinterpret_cast<const float4 *>(src + j);
        const float o[4] = {v.x, v.y, v.z, v.w};
        store_pack<T, 4>(dst + j, o);
    }
    const float *bp = bpart + (((long)b * K + k) * CT) * N * L + i;
    const float *cp = cpart + (((long)b * K + k) * CT) * N * L + i;
    float *grow = gseq + (((long)b * K + k) * L + i) * RG + R8;
    for (int j0 = 0; j0 < BC; j0 += 4) {
        float o[4];
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const int j = j0 + e;
            float sv = 0.f;
            if (j < 2 * N) {
                const float *q = (j < N ? bp + (long)j * L : cp + (long)(j - N) * L);
                for (int t = 0; t < CT; ++t) sv += q[(long)t * N * L];   // fixed order: reproducible
            }
            o[e] = sv;
        }
        *reinterpret_cast<float4 *>(grow + j0) = make_float4(o[0], o[1], o[2], o[3]);
    }
}

// block = 4 waves, wave = one pixel; lane j < RG walks the pixel's CSR entries (ascending entry = ascending direction)
// and keeps the running sum of ITS column for the current direction; out (B, L, K*RG) T.
template <typename T>
__global__ __launch_bounds__(256) void ss2d_bwd_assemble_kernel(const float *__restrict__ gseq,
                                                               const int32_t *__restrict__ inv_ptr,
                                                               const int32_t *__restrict__ inv_idx, T *__restrict__ out,
                                                               long npix, int L, int K, int R, int R8, int N, int BC)
{
    const int lane = threadIdx.x & (kWave - 1);
    const long wid = (long)blockIdx.x * (blockDim.x >> 6) + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    if (wid >= npix) return;
    const int b = (int)((unsigned long)wid / (unsigned)L), p = (int)((unsigned long)wid % (unsigned)L);
    const int RG = R8 + BC;
    const int e0 = __builtin_amdgcn_readfirstlane(inv_ptr[p]), e1 = __builtin_amdgcn_readfirstlane(inv_ptr[p + 1]);
    const float *gb = gseq + (long)b * K * L * RG;
    T *orow = out + ((long)b * L + p) * (long)(K * RG);
    // a lane owns column `lane` (and lane + 64 when RG > 64) of every direction group; columns R .. R8 - 1 (rank padding)
    // and R8 + 2N .. RG - 1 leave as zeros.  The entry list is fetched 64 per load, the rows 8 per batch (all in flight
    // before any is added); entries ascend, i.e. they are grouped by direction: a group's sums leave when the next begins.
    const int l1 = lane + kWave;
    const bool col0 = lane < RG, col1 = l1 < RG;
    const bool live0 = lane < R || (lane >= R8 && lane < R8 + 2 * N);
    const bool live1 = l1 < R || (l1 >= R8 && l1 < R8 + 2 * N);
    float a0 = 0.f, a1 = 0.f;
    int k = 0;
    auto flush = [&]() {
        if (col0) orow[k * RG + lane] = Cvt<T>::from_f(live0 ? a0 : 0.f);
        if (col1) orow[k * RG + l1] = Cvt<T>::from_f(live1 ? a1 : 0.f);
        a0 = a1 = 0.f;
        ++k;
    };
    const int n = e1 - e0;
    for (int base = 0; base < n; base += kWave) {
        const int cn = n - base < kWave ? n - base : kWave;
        const int ent = inv_idx[e0 + base + (lane < cn ? lane : cn - 1)];
        for (int j0 = 0; j0 < cn; j0 += 8) {
            float v0[8], v1[8];
            int ek[8];
#pragma unroll
            for (int jj = 0; jj < 8; ++jj) {
                ek[jj] = __builtin_amdgcn_readlane(ent, j0 + jj < cn ? j0 + jj : cn - 1);
                const float *row = gb + (long)ek[jj] * RG;    // entry = k * L + i
                v0[jj] = col0 ? row[lane] : 0.f;
                v1[jj] = col1 ? row[l1] : 0.f;
            }
#pragma unroll
            for (int jj = 0; jj < 8; ++jj) {
                if (j0 + jj < cn) {   // wave-uniform
                    while (ek[jj] >= (k + 1) * L) flush();
                    a0 += v0[jj];
                    a1 += v1[jj];
                }
            }
        }
    }
    while (k < K) flush();
}

// ------------------------------------------------------------------------------------------------ depth-wise gradients
// gwt (ks*ks + 1, C) f32 = tap-major weight gradient + bias row (tramba_dwconv_wgrad_cl + tramba_slab_sum).
// single stencil:  g7 (C, ks*ks) = transpose of the taps;  gb7 (C) = bias row
// multi-scale (ks = 7, g5 / g3 given): the folded stencil's gradient restricted to each parameter's support
__device__ __forceinline__ void dw_unpack_body(const float *__restrict__ gwt, float *__restrict__ g7, float *__restrict__ g5,
                                               float *__restrict__ g3, float *__restrict__ gb, int nb, int C, int ks, int c)
{
    if (c >= C) return;
    for (int dy = 0; dy < ks; ++dy)
        for (int dx = 0; dx < ks; ++dx) {
            const float v = gwt[(long)(dy * ks + dx) * C + c];
            g7[(long)c * ks * ks + dy * ks + dx] = v;
            if (g5) {
                const int y5 = dy - 1, x5 = dx - 1, y3 = dy - 2, x3 = dx - 2;
                if (y5 >= 0 && y5 < 5 && x5 >= 0 && x5 < 5) g5[(long)c * 25 + y5 * 5 + x5] = v;
                if (y3 >= 0 && y3 < 3 && x3 >= 0 && x3 < 3) g3[(long)c * 9 + y3 * 3 + x3] = v;
            }
        }
    if (gb)   // nb copies of the bias gradient: the folded stencil's bias is the SUM of the three parameters' biases
        for (int q = 0; q < nb; ++q) gb[(long)q * C + c] = gwt[(long)ks * ks * C + c];
}

__global__ __launch_bounds__(256) void dw_unpack_grad_kernel(const float *__restrict__ gwt, float *__restrict__ g7,
                                                            float *__restrict__ g5, float *__restrict__ g3,
                                                            float *__restrict__ gb, int nb, int C, int ks)
{
    dw_unpack_body(gwt, g7, g5, g3, gb, nb, C, ks, blockIdx.x * blockDim.x + threadIdx.x);
}

// the unpacks of a whole backward pass in one launch (the gradients are leaves: nothing reads them before the optimizer);
// items by value, blockIdx.y = item
constexpr int kDwUnpackMulti = 64;
struct DwUnpackItem {
    const float *gwt;
    float *g7, *g5, *g3, *gb;
    int nb, c, ks, pad;
};
struct DwUnpackArgs {
    DwUnpackItem it[kDwUnpackMulti];
};
static_assert(sizeof(DwUnpackArgs) <= 4096, "kernel arguments are limited to 4 KB");
__global__ __launch_bounds__(256) void dw_unpack_multi_kernel(DwUnpackArgs a)
{
    const DwUnpackItem it = a.it[blockIdx.y];
    dw_unpack_body(it.gwt, it.g7, it.g5, it.g3, it.gb, it.nb, it.c, it.ks, blockIdx.x * blockDim.x + threadIdx.x);
}


// ------------------------------------------------------------------------------------------------ C -> 1 head, backward
// y[row] = <x[row, :], w> + b (tramba_rowdot_cl: the decoder's seg_layers, Trambav6.py:82,130).  One pass over x:
//   gx[row, :] = gy[row] * w            (dtype)
//   part[block][0 .. C) += gy[row] * x[row, :],  part[block][C] += gy[row]     (fp32 partial rows, summed by the caller)
// LPR lanes per row (C <= 64 V), 64 / LPR rows of a wave in flight; a wave walks rpw rows.
template <typename T, int V, int LPR>
__global__ __launch_bounds__(256) void rowdot_bwd_kernel(const T *__restrict__ x, const float *__restrict__ gy,
                                                        const float *__restrict__ w, T *__restrict__ gx,
                                                        float *__restrict__ part, long rows, int C, int rpw)
{
    constexpr int RPW = kWave / LPR;
    __shared__ float red[4][LPR * V + 4];
    const int lane = threadIdx.x & (kWave - 1);
    const int wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const long wave = (long)blockIdx.x * (blockDim.x >> 6) + wv;
    const long r0 = wave * rpw;
    const long rend = r0 + rpw < rows ? r0 + rpw : rows;
    const int sub = lane % LPR, slot = lane / LPR;   // (its own lane lines: RowLane cost the fp32 LPR = 64 form 2 SGPRs)
    const int c0 = sub * V;
    const bool cok = c0 + V <= C;
    float wv_[V], gw[V], gb = 0.f;
#pragma unroll
    for (int v = 0; v < V; ++v) {
        wv_[v] = cok ? w[c0 + v] : 0.f;
        gw[v] = 0.f;
    }
    for (long rb = r0; rb < rend; rb += RPW) {
        const long r = rb + slot;
        const bool ok = r < rend && cok;
        float xv[V];
#pragma unroll
        for (int v = 0; v < V; ++v) xv[v] = 0.f;
        float g = 0.f;
        if (ok) {
            load_pack<T, V>(x + r * C + c0, xv);
            g = gy[r];
            float o[V];
#pragma unroll
            for (int v = 0; v < V; ++v) o[v] = g * wv_[v];
            store_pack<T, V>(gx + r * C + c0, o);
        }
#pragma unroll
        for (int v = 0; v < V; ++v) gw[v] = fmaf(g, xv[v], gw[v]);
        if (sub == 0) gb += g;
    }
#pragma unroll
    for (int o = LPR; o < kWave; o <<= 1) {   // fold the row slots of the wave (lanes with equal `sub`)
#pragma unroll
        for (int v = 0; v < V; ++v) gw[v] += __shfl_xor(gw[v], o, kWave);
        gb += __shfl_xor(gb, o, kWave);
    }
    if (slot == 0) {
#pragma unroll
        for (int v = 0; v < V; ++v) red[wv][c0 + v] = gw[v];
        if (sub == 0) red[wv][LPR * V] = gb;
    }
    __syncthreads();
    float *pw = part + (long)blockIdx.x * (C + 4);
    for (int i = threadIdx.x; i < C + 4; i += 256) {
        const int j = i < C ? i : LPR * V + (i - C);
        pw[i] = i <= C ? (red[0][j] + red[1][j]) + (red[2][j] + red[3][j]) : 0.f;
    }
}

// ------------------------------------------------------------------------------------------------ z gate, backward
// p = gelu(n) * silu(z) (SS2D's gated output, vmamba.py:288-290), both operands as stored pre-activations:
//   gn = gp * silu(z) * gelu'(n),   gz = gp * gelu(n) * silu'(z)
// Pointwise, one 16-byte pack per thread and tensor (three reads, two writes per element); the last pack's thread walks the
// count % V tail element by element.  gn or gz may BE gp (a thread reads its elements before it writes them: no __restrict__
// on the three).
template <typename T>
__global__ __launch_bounds__(256) void gelu_gate_bwd_kernel(const T *gp, const T *__restrict__ n, const T *__restrict__ z,
                                                           T *gn, T *gz, long count)
{
    constexpr int V = 16 / (int)sizeof(T);
    const long i0 = ((long)blockIdx.x * blockDim.x + threadIdx.x) * V;
    if (i0 >= count) return;
    if (i0 + V <= count) {
        float g[V], nv[V], zv[V], on[V], oz[V];
        load_pack<T, V>(gp + i0, g);
        load_pack<T, V>(n + i0, nv);
        load_pack<T, V>(z + i0, zv);
#pragma unroll
        for (int v = 0; v < V; ++v) {
            on[v] = g[v] * siluf_(zv[v]) * gelu_gradf_(nv[v]);
            oz[v] = g[v] * geluf_(nv[v]) * silu_gradf_(zv[v]);
        }
        store_pack<T, V>(gn + i0, on);
        store_pack<T, V>(gz + i0, oz);
        return;
    }
    for (long i = i0; i < count; ++i) {
        const float g = Cvt<T>::to_f(gp[i]), nv = Cvt<T>::to_f(n[i]), zv = Cvt<T>::to_f(z[i]);
        gn[i] = Cvt<T>::from_f(g * siluf_(zv) * gelu_gradf_(nv));
        gz[i] = Cvt<T>::from_f(g * geluf_(nv) * silu_gradf_(zv));
    }
}

static long rowdot_bwd_rpw(long rows)
{
    long rpw = rows / 4096;
    return rpw < 8 ? 8 : (rpw > 256 ? 256 : rpw);
}

}  // namespace tramba

using namespace tramba;

extern "C" int tramba_add_layernorm_cl(const void *x, const void *y, const float *mask, int64_t rows_per_sample,
                                       const float *w, const float *b, void *xsum, void *n, void *n_act, int64_t rows,
                                       int c, float eps, int act, int dtype, void *stream)
{
    TRAMBA_CHECK(x && w && b && n, "add_layernorm_cl: null tensor");
    TRAMBA_CHECK(rows > 0 && c > 0, "add_layernorm_cl: empty shape");
    TRAMBA_CHECK(!y || xsum, "add_layernorm_cl: the sum x + y * mask needs an output tensor");
    TRAMBA_CHECK(!mask || rows_per_sample > 0, "add_layernorm_cl: rows_per_sample must be positive with a mask");
    TRAMBA_CHECK(aligned16(x) && aligned16(n) && (!y || (aligned16(y) && aligned16(xsum))) && (!n_act || aligned16(n_act)),
                 "add_layernorm_cl: tensors must be 16-byte aligned");
    ProfScope prof(TRAMBA_PROF_LAYERNORM, (hipStream_t)stream,
                   (2.0 + (y ? 2.0 : 0.0) + (n_act ? 1.0 : 0.0)) * (double)rows * c * dtype_size(dtype));
    TRAMBA_DISPATCH_DTYPE(dtype, T, return launch_add_ln<T>(x, y, mask, rows_per_sample > 0 ? rows_per_sample : 1, w, b, xsum,
                                                            n, n_act, rows, c, dtype, eps, act, (hipStream_t)stream));
    return TRAMBA_OK;
}

extern "C" int tramba_add_layernorm_gate_cl(const void *x, const void *y, const float *mask, int64_t rows_per_sample,
                                            const float *w, const float *b, const void *zpre, void *xsum, void *n,
                                            void *n_act, int64_t rows, int c, float eps, int act, int dtype, void *stream)
{
    TRAMBA_CHECK(x && w && b && n && n_act && zpre, "add_layernorm_gate_cl: null tensor");
    TRAMBA_CHECK(rows > 0 && c > 0, "add_layernorm_gate_cl: empty shape");
    TRAMBA_CHECK(!y || xsum, "add_layernorm_gate_cl: the sum x + y * mask needs an output tensor");
    TRAMBA_CHECK(!mask || rows_per_sample > 0, "add_layernorm_gate_cl: rows_per_sample must be positive with a mask");
    TRAMBA_CHECK(aligned16(x) && aligned16(n) && (!y || (aligned16(y) && aligned16(xsum))) && aligned16(n_act) && aligned16(zpre),
                 "add_layernorm_gate_cl: tensors must be 16-byte aligned");
    ProfScope prof(TRAMBA_PROF_LAYERNORM, (hipStream_t)stream, (4.0 + (y ? 2.0 : 0.0)) * (double)rows * c * dtype_size(dtype));
    TRAMBA_DISPATCH_DTYPE(dtype, T, return launch_add_ln<T>(x, y, mask, rows_per_sample > 0 ? rows_per_sample : 1, w, b, xsum,
                                                            n, n_act, rows, c, dtype, eps, act, (hipStream_t)stream, zpre));
    return TRAMBA_OK;
}

extern "C" int tramba_gelu_gate_bwd_cl(const void *gp, const void *n, const void *zpre, void *gn, void *gz, int64_t count,
                                       int dtype, void *stream)
{
    TRAMBA_CHECK(gp && n && zpre && gn && gz, "gelu_gate_bwd_cl: null tensor");
    TRAMBA_CHECK(count > 0 && count < 2147483648LL, "gelu_gate_bwd_cl: count must be in 1 .. 2^31 - 1");
    TRAMBA_CHECK(aligned16(gp) && aligned16(n) && aligned16(zpre) && aligned16(gn) && aligned16(gz),
                 "gelu_gate_bwd_cl: tensors must be 16-byte aligned");
    const int v = 16 / (int)dtype_size(dtype);
    const long packs = ((long)count + v - 1) / v;
    dim3 grid((unsigned)((packs + 255) / 256)), block(256);
    TRAMBA_DISPATCH_DTYPE(dtype, T,
        hipLaunchKernelGGL((gelu_gate_bwd_kernel<T>), grid, block, 0, (hipStream_t)stream, (const T *)gp, (const T *)n,
                           (const T *)zpre, (T *)gn, (T *)gz, (long)count));
    TRAMBA_LAUNCH_CHECK();
    return TRAMBA_OK;
}

extern "C" int tramba_ss2d_bwd_prep_n_cl(const float *xdbl, const int32_t *table, const float *bpart, const float *cpart,
                                         void *ranks, float *gseq, int batch, int l, int k, int r, int n, int ctiles, int dtype,
                                         void *stream)
{
    TRAMBA_CHECK(xdbl && table && bpart && cpart && ranks && gseq, "ss2d_bwd_prep_cl: null tensor");
    TRAMBA_CHECK(batch > 0 && l > 0 && k > 0 && r > 0 && ctiles > 0 && batch <= 65535 && k <= 65535,
                 "ss2d_bwd_prep_cl: bad shape");
    TRAMBA_CHECK(n >= 1 && n <= 16, "ss2d_bwd_prep_cl: d_state %d outside 1..16", n);
    TRAMBA_CHECK(aligned16(xdbl) && aligned16(ranks) && aligned16(gseq), "ss2d_bwd_prep_cl: 16-byte alignment");
    const int r8 = (r + 7) & ~7, bc = (2 * n + 3) & ~3;
    dim3 grid((unsigned)((l + 255) / 256), (unsigned)k, (unsigned)batch), block(256);
    TRAMBA_DISPATCH_DTYPE(dtype, T,
        hipLaunchKernelGGL((ss2d_bwd_prep_kernel<T>), grid, block, 0, (hipStream_t)stream, xdbl, table, bpart, cpart,
                           (T *)ranks, gseq, l, k, r8, ctiles, n, bc));
    TRAMBA_LAUNCH_CHECK();
    return TRAMBA_OK;
}

extern "C" int tramba_ss2d_bwd_prep_cl(const float *xdbl, const int32_t *table, const float *bpart, const float *cpart,
                                       void *ranks, float *gseq, int batch, int l, int k, int r, int ctiles, int dtype,
                                       void *stream)
{
    return tramba_ss2d_bwd_prep_n_cl(xdbl, table, bpart, cpart, ranks, gseq, batch, l, k, r, 1, ctiles, dtype, stream);
}

extern "C" int tramba_ss2d_bwd_assemble_n_cl(const float *gseq, const int32_t *inv_ptr, const int32_t *inv_idx, void *out,
                                             int batch, int l, int k, int r, int n, int dtype, void *stream)
{
    TRAMBA_CHECK(gseq && inv_ptr && inv_idx && out, "ss2d_bwd_assemble_cl: null tensor");
    TRAMBA_CHECK(batch > 0 && l > 0 && k > 0 && r > 0, "ss2d_bwd_assemble_cl: bad shape");
    TRAMBA_CHECK(n >= 1 && n <= 16, "ss2d_bwd_assemble_cl: d_state %d outside 1..16", n);
    const int r8 = (r + 7) & ~7, bc = (2 * n + 3) & ~3;
    TRAMBA_CHECK(r8 + bc <= 2 * kWave, "ss2d_bwd_assemble_cl: dt_rank %d too large", r);
    const long npix = (long)batch * l;
    TRAMBA_CHECK(npix < 2147483647L, "ss2d_bwd_assemble_cl: too many pixels");
    dim3 grid((unsigned)((npix + 3) / 4)), block(256);
    TRAMBA_DISPATCH_DTYPE(dtype, T,
        hipLaunchKernelGGL((ss2d_bwd_assemble_kernel<T>), grid, block, 0, (hipStream_t)stream, gseq, inv_ptr, inv_idx,
                           (T *)out, npix, l, k, r, r8, n, bc));
    TRAMBA_LAUNCH_CHECK();
    return TRAMBA_OK;
}

extern "C" int tramba_ss2d_bwd_assemble_cl(const float *gseq, const int32_t *inv_ptr, const int32_t *inv_idx, void *out,
                                           int batch, int l, int k, int r, int dtype, void *stream)
{
    return tramba_ss2d_bwd_assemble_n_cl(gseq, inv_ptr, inv_idx, out, batch, l, k, r, 1, dtype, stream);
}

extern "C" int tramba_dw_unpack_grad(const float *gwt, float *g7, float *g5, float *g3, float *gb, int nb, int c, int ks,
                                     void *stream)
{
    TRAMBA_CHECK(gwt && g7 && c > 0, "dw_unpack_grad: null tensor");
    TRAMBA_CHECK(ks == 3 || ks == 5 || ks == 7, "dw_unpack_grad: kernel size %d unsupported (3,5,7)", ks);
    TRAMBA_CHECK((g5 == nullptr) == (g3 == nullptr) && (!g5 || ks == 7), "dw_unpack_grad: multi-scale needs ks = 7, g5 and g3");
    hipLaunchKernelGGL(dw_unpack_grad_kernel, dim3((c + 255) / 256), dim3(256), 0, (hipStream_t)stream, gwt, g7, g5, g3, gb,
                       nb, c, ks);
    TRAMBA_LAUNCH_CHECK();
    return TRAMBA_OK;
}

extern "C" int tramba_dw_unpack_grad_multi(const float *const *gwt, float *const *g7, float *const *g5, float *const *g3,
                                           float *const *gb, const int *nb, const int *c, const int *ks, int count, void *stream)
{
    TRAMBA_CHECK(gwt && g7 && g5 && g3 && gb && nb && c && ks && count > 0, "dw_unpack_grad_multi: empty input");
    for (int base = 0; base < count; base += kDwUnpackMulti) {
        DwUnpackArgs a;
        const int n = count - base < kDwUnpackMulti ? count - base : kDwUnpackMulti;
        int cmax = 0;
        for (int i = 0; i < kDwUnpackMulti; ++i) {
            const int j = base + (i < n ? i : 0);
            TRAMBA_CHECK(gwt[j] && g7[j] && c[j] > 0, "dw_unpack_grad_multi: item %d: null tensor", j);
            TRAMBA_CHECK(ks[j] == 3 || ks[j] == 5 || ks[j] == 7, "dw_unpack_grad_multi: item %d: kernel size %d unsupported", j, ks[j]);
            TRAMBA_CHECK((g5[j] == nullptr) == (g3[j] == nullptr) && (!g5[j] || ks[j] == 7),
                         "dw_unpack_grad_multi: item %d: multi-scale needs ks = 7, g5 and g3", j);
            a.it[i] = DwUnpackItem{gwt[j], g7[j], g5[j], g3[j], gb[j], nb[j], c[j], ks[j], 0};
            if (i < n && c[j] > cmax) cmax = c[j];
        }
        hipLaunchKernelGGL(dw_unpack_multi_kernel, dim3((cmax + 255) / 256, n), dim3(256), 0, (hipStream_t)stream, a);
        TRAMBA_LAUNCH_CHECK();
    }
    return TRAMBA_OK;
}

// the backward holds a whole row in one pack per lane like the LayerNorm kernels (row_form, not the forward's dividing rule)
static RowPlan rowdot_bwd_plan(long rows, int c, int dtype)
{
    RowPlan p{row_form(c, dtype), 0, 0};
    if (rows <= 0 || c <= 0 || !p.form.ok) return p;     // parts 0: shape not served by this kernel
    p.per_wave = rowdot_bwd_rpw(rows);
    p.parts = rows_grid((rows + p.per_wave - 1) / p.per_wave);
    return p;
}

extern "C" int64_t tramba_rowdot_bwd_parts(int64_t rows, int c, int dtype) { return rowdot_bwd_plan(rows, c, dtype).parts; }

extern "C" int tramba_rowdot_bwd_cl(const void *x, const float *gy, const float *w, void *gx, float *part, int64_t rows,
                                    int c, int dtype, void *stream)
{
    TRAMBA_CHECK(x && gy && w && gx && part, "rowdot_bwd_cl: null tensor");
    const RowPlan plan = rowdot_bwd_plan(rows, c, dtype);
    TRAMBA_CHECK(plan.parts > 0, "rowdot_bwd_cl: C=%d is not served (rows of at most 64 x 16 bytes)", c);
    TRAMBA_CHECK(aligned16(x) && aligned16(gx) && aligned16(w), "rowdot_bwd_cl: tensors must be 16-byte aligned");
    hipStream_t s = (hipStream_t)stream;
    const dim3 grid((unsigned)plan.parts), block(256);
    TRAMBA_DISPATCH_DTYPE(dtype, T, with_lpr(plan.form.lpr, [&](auto L) {
        hipLaunchKernelGGL((rowdot_bwd_kernel<T, kRowVec<T>, decltype(L)::value>), grid, block, 0, s, (const T *)x, gy, w,
                           (T *)gx, part, (long)rows, c, (int)plan.per_wave);
    }));
    TRAMBA_LAUNCH_CHECK();
    return TRAMBA_OK;
}
