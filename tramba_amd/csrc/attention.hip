// Fused attention for the Swin-B / PVTv2-b4 encoders of Tramba-S / Tramba-P (inference, 16-bit).
//
// One kernel core, two gathers.  An attention problem here is small: at most 256 keys of head dim 32 or 64 (Swin: the
// ws x ws tokens of one window; PVT: the spatially reduced map), so K and V of one (problem, head) sit in LDS whole and
// there is no K/V tile loop and no online softmax.  A workgroup (4 waves) takes one (problem, head) and a run of
// 16-query tiles; each wave works on one tile at a time:
//
//   S^T = K Q^T      mfma_16x16x32(A = K rows from LDS, B = Q rows from global): the accumulator of key tile t holds, in
//                    lane (g = lane >> 4, q = lane & 15), the scores of query q against keys 16 t + 4 g + r, r = 0..3.
//                    A score row is spread over the 4 lanes of one q: row max / sum = registers, then two xor-shuffles.
//   softmax          f32, exp2 with log2(e) folded into the f32 scale; the scale multiplies the ACCUMULATED score.
//   O^T = V^T P^T    the score accumulators, rounded to the dtype, are the B operand as they lie (k-step s = key tiles
//                    2 s and 2 s + 1, so element j of lane group g is key 32 s + 16 (j >> 2) + 4 g + (j & 3)); the A
//                    operand takes V in that same key order from a transposed LDS image Vt[d][key].  f32 accumulation,
//                    divided by the f32 row sum, rounded once.
//
// No atomics and a fixed summation order: bitwise reproducible.  No allocation, no synchronisation: capturable.
#include "common.h"

namespace tramba {

typedef __attribute__((ext_vector_type(8))) short at_frag8;
typedef __attribute__((ext_vector_type(4))) short at_frag4;
typedef __attribute__((ext_vector_type(4))) float at_acc4;
typedef __attribute__((ext_vector_type(4))) int at_int4;
typedef __attribute__((ext_vector_type(4))) unsigned at_u4;

template <typename T> struct AtMfma;
template <> struct AtMfma<__hip_bfloat16> {
    static __device__ __forceinline__ at_acc4 run(at_frag8 a, at_frag8 b, at_acc4 c)
    {
        typedef __attribute__((ext_vector_type(8))) __bf16 bf8;
        return __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf8, a), __builtin_bit_cast(bf8, b), c, 0, 0, 0);
    }
};
template <> struct AtMfma<__half> {
    static __device__ __forceinline__ at_acc4 run(at_frag8 a, at_frag8 b, at_acc4 c)
    {
        typedef __attribute__((ext_vector_type(8))) _Float16 h8;
        return __builtin_amdgcn_mfma_f32_16x16x32_f16(__builtin_bit_cast(h8, a), __builtin_bit_cast(h8, b), c, 0, 0, 0);
    }
};

template <typename T> __device__ __forceinline__ short at_round(float v)
{
    const T t = Cvt<T>::from_f(v);          // round to nearest even
    return __builtin_bit_cast(short, t);
}

struct AttnArgs {
    const void *q, *k, *v;   // row r of a tensor starts at base + r * ld elements; the head adds h * HD
    void *y;
    const float *table;      // window form: ((2 ws - 1)^2, heads) f32
    long q_ld, kv_ld, y_ld;
    int nq, nk;              // queries / keys of one problem
    int heads, cpw, split;   // 16-query tiles per workgroup, workgroups per (problem, head)
    int h, w, ws, shift, nwx, nwy;
    float scale2;            // hd^-0.5 * log2(e)
};

constexpr float kLog2e = 1.44269504088896340736f;
constexpr int kAttnThreads = 256;

// NT2 = 32-key steps of P V (the keys are padded to 32 NT2; pad keys score -inf and carry zero K / V)
template <typename T, int HD, int NT2, bool WIN>
__global__ __launch_bounds__(kAttnThreads) void attn_kernel(AttnArgs a)
{
    constexpr int NK = NT2 * 32, NT = NT2 * 2;
    constexpr int KS = HD * 2 + 16;            // bytes per K row: 16 rows at one 16-byte chunk fall on 16 distinct slots of 256 B
    constexpr int VS = NK * 2 + 16;            // bytes per Vt row: likewise for the 8-byte reads of 16 d rows x 2 lane groups
    constexpr int CH = HD / 8;                 // 16-byte chunks per head row
    constexpr int WSMAX = NT2 == 2 ? 8 : (NT2 == 5 ? 12 : 16);
    constexpr int NB = WIN ? (2 * WSMAX - 1) * (2 * WSMAX - 1) : 1;
    __shared__ __attribute__((aligned(16))) unsigned char k_lds[NK * KS];
    __shared__ __attribute__((aligned(16))) unsigned char v_lds[HD * VS];
    __shared__ float bias_lds[NB];                                   // this head's table column, times log2(e)
    __shared__ int tok_lds[WIN ? NK : 1];                            // token -> y * W + x through the cyclic shift
    __shared__ __attribute__((aligned(16))) int meta_lds[WIN ? NK : 4];   // token -> (i (2 ws - 1) + j) | region id << 16

    unsigned item, u1, u2;
    xcd_work_item(item, u1, u2);
    const int chunk = item % a.split;
    const int ph = item / a.split;
    const int head = ph % a.heads, prob = ph / a.heads;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int nk = a.nk, nq = a.nq;

    long qbase, kbase;
    if constexpr (WIN) {
        const int ws = a.ws, nw = a.nwx * a.nwy;
        const int b = prob / nw, wi = prob % nw;
        const int wy = wi / a.nwx, wx = wi % a.nwx;
        for (int n = tid; n < NK; n += kAttnThreads) {
            int tok = 0, meta = 0;
            if (n < nk) {
                const int i = n / ws, j = n % ws;
                const int ry = wy * ws + i, rx = wx * ws + j;        // rolled-frame coordinates
                int y = ry + a.shift, x = rx + a.shift;
                y = y >= a.h ? y - a.h : y;
                x = x >= a.w ? x - a.w : x;
                tok = y * a.w + x;
                int rid = 0;
                if (a.shift > 0) {
                    const int r = ry < a.h - ws ? 0 : (ry < a.h - a.shift ? 1 : 2);
                    const int c = rx < a.w - ws ? 0 : (rx < a.w - a.shift ? 1 : 2);
                    rid = 3 * r + c;
                }
                meta = (i * (2 * ws - 1) + j) | (rid << 16);
            }
            tok_lds[n] = tok;
            meta_lds[n] = meta;
        }
        const int nb = (2 * ws - 1) * (2 * ws - 1);
        for (int e = tid; e < nb; e += kAttnThreads) bias_lds[e] = a.table[(long)e * a.heads + head] * kLog2e;
        qbase = kbase = (long)b * a.h * a.w;
        __syncthreads();
    } else {
        qbase = (long)prob * nq;
        kbase = (long)prob * nk;
    }

    const T *qp = static_cast<const T *>(a.q) + head * HD;
    const T *kp = static_cast<const T *>(a.k) + head * HD;
    const T *vp = static_cast<const T *>(a.v) + head * HD;
    T *yp = static_cast<T *>(a.y) + head * HD;

    // K as it lies, [key][d]; V transposed, [d][key]; pad keys zero (0 * P = 0, never NaN)
    for (int e = tid; e < NK * CH; e += kAttnThreads) {
        const int m = e / CH, c = e % CH;
        at_u4 kk = {0u, 0u, 0u, 0u}, vv = {0u, 0u, 0u, 0u};
        if (m < nk) {
            long row = kbase;
            if constexpr (WIN) row += tok_lds[m]; else row += m;
            kk = *reinterpret_cast<const at_u4 *>(kp + row * a.kv_ld + c * 8);
            vv = *reinterpret_cast<const at_u4 *>(vp + row * a.kv_ld + c * 8);
        }
        *reinterpret_cast<at_u4 *>(k_lds + m * KS + c * 16) = kk;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            *reinterpret_cast<unsigned short *>(v_lds + (c * 8 + 2 * i) * VS + m * 2) = (unsigned short)(vv[i] & 0xffffu);
            *reinterpret_cast<unsigned short *>(v_lds + (c * 8 + 2 * i + 1) * VS + m * 2) = (unsigned short)(vv[i] >> 16);
        }
    }
    __syncthreads();

    const int g = lane >> 4, li = lane & 15;
    const int cst = (a.ws - 1) * (2 * a.ws - 1) + a.ws - 1;
    for (int tt = wave; tt < a.cpw; tt += kAttnThreads / 64) {
        const int qt = chunk * a.cpw + tt;
        if (qt * 16 >= nq) break;                                   // wave-uniform
        int qn = qt * 16 + li;
        const bool qok = qn < nq;
        qn = qok ? qn : nq - 1;                                     // a ragged tile recomputes the last row and stores nothing
        long qrow = qbase;
        if constexpr (WIN) qrow += tok_lds[qn]; else qrow += qn;

        at_frag8 qf[HD / 32];
#pragma unroll
        for (int ks = 0; ks < HD / 32; ++ks)
            qf[ks] = *reinterpret_cast<const at_frag8 *>(qp + qrow * a.q_ld + ks * 32 + g * 8);

        at_acc4 s[NT];
#pragma unroll
        for (int t = 0; t < NT; ++t) {
            at_acc4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int ks = 0; ks < HD / 32; ++ks) {
                const at_frag8 kf = *reinterpret_cast<const at_frag8 *>(k_lds + (16 * t + li) * KS + (ks * 32 + g * 8) * 2);
                acc = AtMfma<T>::run(kf, qf[ks], acc);
            }
            s[t] = acc;
        }

        int qij = 0, qrid = 0;
        if constexpr (WIN) {
            const int qm = meta_lds[qn];
            qij = (qm & 0xffff) + cst;
            qrid = qm >> 16;
        }
        float mx = -INFINITY;
#pragma unroll
        for (int t = 0; t < NT; ++t) {
            at_int4 km = {0, 0, 0, 0};
            if constexpr (WIN) km = *reinterpret_cast<const at_int4 *>(&meta_lds[16 * t + 4 * g]);
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                float v = s[t][r] * a.scale2;
                if constexpr (WIN) {
                    v += bias_lds[qij - (km[r] & 0xffff)];
                    if ((km[r] >> 16) != qrid) v += -100.f * kLog2e;
                }
                if (16 * t + 4 * g + r >= nk) v = -INFINITY;
                s[t][r] = v;
                mx = fmaxf(mx, v);
            }
        }
        mx = fmaxf(mx, __shfl_xor(mx, 16, 64));
        mx = fmaxf(mx, __shfl_xor(mx, 32, 64));
        float sum = 0.f;
#pragma unroll
        for (int t = 0; t < NT; ++t)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const float p = __builtin_amdgcn_exp2f(s[t][r] - mx);
                s[t][r] = p;
                sum += p;
            }
        sum += __shfl_xor(sum, 16, 64);
        sum += __shfl_xor(sum, 32, 64);

        at_acc4 o[HD / 16];
#pragma unroll
        for (int dt = 0; dt < HD / 16; ++dt) o[dt] = at_acc4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int s2 = 0; s2 < NT2; ++s2) {
            at_frag8 pf;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                pf[r] = at_round<T>(s[2 * s2][r]);
                pf[4 + r] = at_round<T>(s[2 * s2 + 1][r]);
            }
#pragma unroll
            for (int dt = 0; dt < HD / 16; ++dt) {
                const unsigned char *vr = v_lds + (16 * dt + li) * VS + (32 * s2 + 4 * g) * 2;
                const at_frag4 lo = *reinterpret_cast<const at_frag4 *>(vr);
                const at_frag4 hi = *reinterpret_cast<const at_frag4 *>(vr + 32);
                const at_frag8 vf = {lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
                o[dt] = AtMfma<T>::run(vf, pf, o[dt]);
            }
        }
        if (qok) {
            T *yr = yp + qrow * a.y_ld + 4 * g;
#pragma unroll
            for (int dt = 0; dt < HD / 16; ++dt) {
                at_frag4 out;
#pragma unroll
                for (int r = 0; r < 4; ++r) out[r] = at_round<T>(o[dt][r] / sum);
                *reinterpret_cast<at_frag4 *>(yr + 16 * dt) = out;
            }
        }
    }
}

// How one problem's 16-query tiles are dealt to workgroups: about two workgroups per compute unit when the call has that
// many tiles (each workgroup stages K / V once, 18-36 KB from L2), one tile per workgroup when it has fewer, and the
// whole problem in one workgroup only when the (problem, head) pairs alone fill the chip.
static void attn_split(long problems, int qtiles, int &cpw, int &split)
{
    long c = problems * qtiles / 512;
    c = c < 1 ? 1 : (c > qtiles ? qtiles : c);
    cpw = (int)c;
    split = (qtiles + cpw - 1) / cpw;
}

template <typename T, int HD, bool WIN>
static int attn_launch_nt(AttnArgs &a, long problems, hipStream_t s)
{
    const int qtiles = (a.nq + 15) / 16;
    attn_split(problems, qtiles, a.cpw, a.split);
    const long grid = problems * a.split;
    TRAMBA_CHECK(grid > 0 && grid < (1L << 31), "attention: %ld workgroups exceed the grid", grid);
    const dim3 gr((unsigned)grid), bl(kAttnThreads);
    if (a.nk <= 64)
        hipLaunchKernelGGL((attn_kernel<T, HD, 2, WIN>), gr, bl, 0, s, a);
    else if (a.nk <= 160)
        hipLaunchKernelGGL((attn_kernel<T, HD, 5, WIN>), gr, bl, 0, s, a);
    else
        hipLaunchKernelGGL((attn_kernel<T, HD, 8, WIN>), gr, bl, 0, s, a);
    TRAMBA_LAUNCH_CHECK();
    return TRAMBA_OK;
}

template <bool WIN>
static int attn_launch(AttnArgs &a, long problems, int hd, int dtype, hipStream_t s)
{
    a.scale2 = (float)((1.0 / sqrt((double)hd)) * 1.4426950408889634);
    if (dtype == TRAMBA_BF16)
        return hd == 32 ? attn_launch_nt<__hip_bfloat16, 32, WIN>(a, problems, s) : attn_launch_nt<__hip_bfloat16, 64, WIN>(a, problems, s);
    return hd == 32 ? attn_launch_nt<__half, 32, WIN>(a, problems, s) : attn_launch_nt<__half, 64, WIN>(a, problems, s);
}

}  // namespace tramba

using namespace tramba;

extern "C" int tramba_window_attn_cl(const void *qkv, const float *table, void *y, int batch, int h, int w, int heads,
                                     int hd, int ws, int shift, int dtype, void *stream)
{
    TRAMBA_CHECK(qkv && table && y, "window_attn_cl: null tensor");
    TRAMBA_CHECK(dtype == TRAMBA_BF16 || dtype == TRAMBA_F16, "window_attn_cl: dtype %d is not bf16 / fp16", dtype);
    TRAMBA_CHECK(hd == 32 || hd == 64, "window_attn_cl: hd %d is not 32 or 64", hd);
    TRAMBA_CHECK(batch > 0 && h > 0 && w > 0 && heads > 0, "window_attn_cl: empty shape");
    TRAMBA_CHECK(ws >= 1 && ws * ws <= 256, "window_attn_cl: ws %d outside 1..16", ws);
    TRAMBA_CHECK(h % ws == 0 && w % ws == 0, "window_attn_cl: map %d x %d is no multiple of ws %d", h, w, ws);
    TRAMBA_CHECK(shift >= 0 && shift < ws, "window_attn_cl: shift %d outside 0..ws-1", shift);
    TRAMBA_CHECK((long)h * w < (1L << 31), "window_attn_cl: map %d x %d too large", h, w);   // a token's y * W + x is an int
    TRAMBA_CHECK(aligned16(qkv) && aligned16(y), "window_attn_cl: tensors must be 16-byte aligned");
    const long c = (long)heads * hd;
    const size_t es = 2;
    AttnArgs a = {};
    a.q = qkv;
    a.k = static_cast<const char *>(qkv) + c * es;
    a.v = static_cast<const char *>(qkv) + 2 * c * es;
    a.y = y;
    a.table = table;
    a.q_ld = a.kv_ld = 3 * c;
    a.y_ld = c;
    a.nq = a.nk = ws * ws;
    a.heads = heads;
    a.h = h, a.w = w, a.ws = ws, a.shift = shift, a.nwx = w / ws, a.nwy = h / ws;
    return attn_launch<true>(a, (long)batch * a.nwx * a.nwy * heads, hd, dtype, (hipStream_t)stream);
}

extern "C" int tramba_kv_attn_cl(const void *q, const void *kv, void *y, int batch, int64_t n, int m, int heads, int hd,
                                 int dtype, void *stream)
{
    TRAMBA_CHECK(q && kv && y, "kv_attn_cl: null tensor");
    TRAMBA_CHECK(dtype == TRAMBA_BF16 || dtype == TRAMBA_F16, "kv_attn_cl: dtype %d is not bf16 / fp16", dtype);
    TRAMBA_CHECK(hd == 32 || hd == 64, "kv_attn_cl: hd %d is not 32 or 64", hd);
    TRAMBA_CHECK(batch > 0 && heads > 0, "kv_attn_cl: empty shape");
    TRAMBA_CHECK(n >= 1 && n < (1L << 31) - 16, "kv_attn_cl: N %ld outside 1..2^31-17", (long)n);
    TRAMBA_CHECK(m >= 1 && m <= 256, "kv_attn_cl: M %d outside 1..256", m);
    TRAMBA_CHECK(aligned16(q) && aligned16(kv) && aligned16(y), "kv_attn_cl: tensors must be 16-byte aligned");
    const long c = (long)heads * hd;
    AttnArgs a = {};
    a.q = q;
    a.k = kv;
    a.v = static_cast<const char *>(kv) + c * 2;
    a.y = y;
    a.q_ld = a.y_ld = c;
    a.kv_ld = 2 * c;
    a.nq = (int)n, a.nk = m;
    a.heads = heads;
    a.ws = 1;
    return attn_launch<false>(a, (long)batch * heads, hd, dtype, (hipStream_t)stream);
}
