// LayerNorm helpers shared by the norm kernels: the wave form's statistics, and the rows form's plan, dispatch and lanes.
#pragma once
#include <type_traits>

#include "common.h"

namespace tramba {

constexpr int kNormMaxIt = 8;

// One wave normalises one row held as acc[it][v] (channel = (it*64 + lane)*V + v).
template <int V>
__device__ __forceinline__ void wave_layernorm(float (&acc)[kNormMaxIt][V], int nit, int C, int lane,
                                               float eps, float &mean, float &rstd)
{
    float s = 0.f;
#pragma unroll
    for (int it = 0; it < kNormMaxIt; ++it)
        if (it < nit)
#pragma unroll
            for (int v = 0; v < V; ++v)
                if ((it * kWave + lane) * V + v < C) s += acc[it][v];
    mean = wave_sum(s) / (float)C;
    float q = 0.f;
#pragma unroll
    for (int it = 0; it < kNormMaxIt; ++it)
        if (it < nit)
#pragma unroll
            for (int v = 0; v < V; ++v)
                if ((it * kWave + lane) * V + v < C) {
                    const float t = acc[it][v] - mean;
                    q = fmaf(t, t, q);
                }
    rstd = rsqrtf(wave_sum(q) / (float)C + eps);
}

// vector width for a row of C channels: the largest of 8/4/2/1 that divides C and keeps the
// row within kNormMaxIt wave iterations while using as many lanes as possible
inline int norm_vec(int c, int maxv)
{
    int v = maxv;
    while (v > 1 && (c % v != 0 || c / v < kWave)) v >>= 1;
    while ((c + kWave * v - 1) / (kWave * v) > kNormMaxIt && v < maxv && c % (2 * v) == 0) v <<= 1;
    return v;
}

// row q = ((b*H + h)*W + w)*P*P + p1*P + p2 of a (B, H, W, P*P*C) map -> row of output pixel (b, h*P + p1, w*P + p2): the
// pixel shuffle 'b (p1 p2 c) h w -> b c (h p1) (w p2)' in channels-last rows.  32-bit index arithmetic (rows < 2^31,
// host-checked): six emulated 64-bit divisions per lane were most of the forward kernels' instructions
__device__ __forceinline__ long shuffled_row(long row, int P, int H, int W)
{
    if (P <= 1) return row;
    const unsigned r32u = (unsigned)row, pp2 = (unsigned)(P * P);
    const unsigned pp = r32u % pp2, pix = r32u / pp2;
    const unsigned wi = pix % (unsigned)W, bh = pix / (unsigned)W;
    const unsigned hi = bh % (unsigned)H, b = bh / (unsigned)H;
    return ((long)b * (H * P) + (long)(hi * P + pp / P)) * (long)(W * P) + (long)(wi * P + pp % P);
}

// ---- the rows form: LPR lanes per row, 64 / LPR rows of a wave in flight, one 16-byte pack of VM elements per lane
// (C <= 64 * VM; VM = 8 for 16-bit, 4 for fp32).  The host plan, its dispatch and the lane's place are written down here
// once; the kernels keep their own arithmetic around the sums.
struct RowForm {
    int vm, lpr;   // elements of a lane's pack; lanes per row (a power of two, 1 .. 64)
    bool ok;       // the row fits the form
};
template <typename T> constexpr int kRowVec = 16 / (int)sizeof(T);   // vm as the kernels' template argument
// LayerNorm family: one pack per lane covers the row -- lpr = the smallest power of two >= C / vm
inline RowForm row_form(int c, int dtype)
{
    RowForm f{dtype == TRAMBA_F32 ? 4 : 8, 1, false};
    f.ok = c % f.vm == 0 && c / f.vm <= kWave;
    while (f.ok && f.lpr < c / f.vm) f.lpr <<= 1;
    return f;
}
// row-dot forward: a lane strides the row by lpr packs, so lpr * vm has to DIVIDE C -- the largest such power of two <= 64
inline RowForm row_form_dividing(int c, int dtype)
{
    RowForm f{dtype == TRAMBA_F32 ? 4 : 8, 1, false};
    f.ok = c % f.vm == 0;
    while (f.ok && f.lpr < kWave && c % (2 * f.lpr * f.vm) == 0) f.lpr <<= 1;
    return f;
}
inline long rows_waves(long rows, int lpr) { return (rows + (kWave / lpr) - 1) / (kWave / lpr); }   // one row group per wave
inline long rows_grid(long waves) { return (waves + 3) / 4; }                                      // four waves per workgroup
// what a sizing query and its launch have to agree on: both read it from ONE function per kernel
struct RowPlan {
    RowForm form;
    long per_wave;   // rows (or, norm-head backward, row groups) a wave walks
    long parts;      // workgroups = partial rows; 0: the shape is not served
};

// f(std::integral_constant<int, L>{}) for the runtime lpr -- the one switch over the seven forms
template <typename F> inline void with_lpr(int lpr, F &&f)
{
    switch (lpr) {
    case 1: f(std::integral_constant<int, 1>{}); break;
    case 2: f(std::integral_constant<int, 2>{}); break;
    case 4: f(std::integral_constant<int, 4>{}); break;
    case 8: f(std::integral_constant<int, 8>{}); break;
    case 16: f(std::integral_constant<int, 16>{}); break;
    case 32: f(std::integral_constant<int, 32>{}); break;
    default: f(std::integral_constant<int, 64>{}); break;
    }
}
// the same for norm_vec's 8 / 4 / 2 / 1 of the one-row-per-wave form (no fp32 kernel with V = 8 exists)
template <typename T, typename F> inline void with_norm_vec(int v, F &&f)
{
    switch (v) {
    case 8: if constexpr (sizeof(T) == 2) f(std::integral_constant<int, 8>{}); break;
    case 4: f(std::integral_constant<int, 4>{}); break;
    case 2: f(std::integral_constant<int, 2>{}); break;
    default: f(std::integral_constant<int, 1>{}); break;
    }
}

// a lane's place in the form: pack `sub` of row slot `slot`
// (lane and sub are read once and kept, so that every use sees ONE value; the rest are functions, so that each kernel names
// them in the order its body always did -- the compiler's schedule is seeded by that order and stays what it was)
template <int V, int LPR> struct RowLane {
    static constexpr int RPW = kWave / LPR;
    const int lane, sub;
    __device__ __forceinline__ explicit RowLane(int lane_ = threadIdx.x & (kWave - 1)) : lane(lane_), sub(lane_ % LPR) {}
    __device__ __forceinline__ int slot() const { return lane / LPR; }
    __device__ __forceinline__ int c0() const { return sub * V; }
    // the lane's pack lies within the row (false on the idle lanes of a C / V that is no power of two)
    __device__ __forceinline__ bool cok(int C) const { return c0() + V <= C; }
    // the lane's row where every wave takes ONE row group (the looping kernels add slot() to their own group's first row)
    __device__ __forceinline__ long row() const
    {
        const long wave = (long)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
        return wave * RPW + slot();
    }
};
// sum over the LPR lanes of a row; every lane of the row receives it
template <int LPR> __device__ __forceinline__ float sub_sum(float s)
{
#pragma unroll
    for (int o = LPR / 2; o > 0; o >>= 1) s += __shfl_xor(s, o, LPR);
    return s;
}
// SS2D's z gate (vmamba.py:288-290) as the last step of a row epilogue: with GATE the row piece is stored as
// o[v] * silu(g[v]), g = the gate's stored PRE-activation at the channels of o; without it the values are stored as they are
// and g is never touched -- the ungated instantiation of a kernel body does the arithmetic it did, in the same order.
template <typename T, int V, bool GATE>
__device__ __forceinline__ void store_gated(T *p, float (&o)[V], const T *g)
{
    if constexpr (GATE) {
        float zv[V];
        load_pack<T, V>(g, zv);
#pragma unroll
        for (int v = 0; v < V; ++v) o[v] *= siluf_(zv[v]);
    }
    store_pack<T, V>(p, o);
}
// The streaming merge asks for its gate rows AHEAD of the row statistics, so that the load's latency passes under the wave
// reductions: NIT packs through a buffer descriptor over the wave's rows (`rows`, `bytes`: wave-uniform), addressed exactly
// like the output rows (off[it] + row_off; a batch that does not store, `live` false, asks out of range and reads nothing).
// The loop that follows stays branch-free.  Without GATE nothing is requested and the packs are never looked at.
template <typename T, int V, int NIT> struct GatePacks {
    Pack<T, V> p[NIT];
};
template <typename T, int V, int NIT, bool GATE>
__device__ __forceinline__ GatePacks<T, V, NIT> gate_request(const T *rows, unsigned bytes, const unsigned (&off)[NIT], bool live,
                                                            unsigned row_off)
{
    GatePacks<T, V, NIT> g{};
    if constexpr (GATE) {
        constexpr int kB = (int)sizeof(T) * V;
        static_assert(kB == 16 || kB == 8 || kB == 4 || kB == 2, "row piece of 2..16 bytes");
        const __amdgpu_buffer_rsrc_t r = make_rsrc(rows, bytes);
#pragma unroll
        for (int it = 0; it < NIT; ++it) {
            const unsigned vo = (live ? off[it] : kOutOfRange) + row_off;
            if constexpr (kB == 16) g.p[it] = __builtin_bit_cast(Pack<T, V>, __builtin_amdgcn_raw_buffer_load_b128(r, vo, 0, 0));
            else if constexpr (kB == 8) g.p[it] = __builtin_bit_cast(Pack<T, V>, __builtin_amdgcn_raw_buffer_load_b64(r, vo, 0, 0));
            else if constexpr (kB == 4) g.p[it] = __builtin_bit_cast(Pack<T, V>, __builtin_amdgcn_raw_buffer_load_b32(r, vo, 0, 0));
            else g.p[it] = __builtin_bit_cast(Pack<T, V>, __builtin_amdgcn_raw_buffer_load_b16(r, vo, 0, 0));
        }
    }
    return g;
}
// the values of a row piece, times silu of the requested gate pack with GATE, as the pack the buffer store takes
template <typename T, int V, bool GATE>
__device__ __forceinline__ Pack<T, V> pack_gated(float (&o)[V], const Pack<T, V> &g)
{
    Pack<T, V> z;
#pragma unroll
    for (int v = 0; v < V; ++v) z.v[v] = Cvt<T>::from_f(GATE ? o[v] * siluf_(Cvt<T>::to_f(g.v[v])) : o[v]);
    return z;
}

}  // namespace tramba
