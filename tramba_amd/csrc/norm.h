// Wave-level LayerNorm helper shared by the norm kernels.
#pragma once
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
