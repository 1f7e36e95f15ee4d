// Attention backward for the Swin-B / PVTv2-b4 encoders of Tramba-S / Tramba-P (training, 16-bit): the other half of
// attention.hip.  Nothing is saved by the forward: the kernel takes q, k, v, the bias table and dO and recomputes the
// softmax rows.  K and V of one (problem, head) sit in LDS whole, row-major, as in the forward.
//
// A workgroup (4 waves) takes one (problem, head) and a run of ROUNDS of QR = 64 queries (32 at the 256-key cap, where
// LDS is short).  A round has two phases:
//
//  A  each wave takes one 16-query tile (lane (g = lane >> 4, q = lane & 15), registers = keys 16 t + 4 g + r, the
//     forward's layout):
//       S^T  = K Q^T          A = K rows (LDS), B = Q rows (global)         -> P = softmax, f32, normalised by the f32 row sum
//       dP^T = V dO^T         A = V rows (LDS), B = dO rows (global)        -> the same lane layout as S^T
//       D    = sum_k P dP     registers, then two xor-shuffles
//       dS   = P (dP - D)     f32
//       dQ^T = K^T dS^T       B = dS as it lies, split into two 16-bit operands (hi = round(dS), lo = round(dS - hi), two
//                             MFMAs); A = K read TRANSPOSED from the row-major image (ds_read_b64_tr_b16), in the
//                             forward's permuted key order; scaled in f32, stored once
//     and leaves in LDS, for phase B: the Q and dO rows as loaded, and P and dS in f32 as [query][key] images.
//  B  dV = P^T dO and dK = dS^T Q contract over the query, the LANE index of phase A, hence the trip through LDS: each wave
//     owns the key tiles t = wave, wave + 4, ... and keeps their f32 accumulators in registers over ALL rounds of the
//     workgroup.  A = a column of the f32 [query][key] image, split hi / lo as above; B = the [query][d] rows of dO / Q
//     by transposed reads.
//     P and dS are split because one 16-bit rounding of them is what separates this kernel from the stock autograd path,
//     whose attention math runs in f32: with it the qkv weight gradient of a block carried 2.9 % more error than stock's,
//     against a stock seed-to-seed spread of 2.5 % (profiles/attn_train_parity.json).  The price is 8 MFMAs where 5 would do.
//     dtable: a thread owns bins e = tid, tid + 256, ...; for bin (di, dj) and query (i, j) the key (i - di, j - dj) is
//     unique, so the thread adds at most one f32 dS per query, in query order.  No atomics.
//
// Window form: a workgroup holds a whole window (every token lies in exactly one), so dK and dV are complete in its
// registers and are scaled, rounded and written through the cyclic shift.  The per-workgroup bin sums go to the workspace
// and a second launch adds them over (batch, window) in index order.
// kv form: the N queries of a (batch, head) are dealt to `split` workgroups; each writes its f32 dK / dV partial to the
// workspace and a second launch adds them in chunk order, scales dK, rounds once and writes dkv.
//
// Fixed summation order everywhere: bitwise reproducible.  No allocation, no synchronisation: capturable.
#include "common.h"

namespace tramba {

typedef __attribute__((ext_vector_type(8))) short ab_frag8;
typedef __attribute__((ext_vector_type(4))) short ab_frag4;
typedef __attribute__((ext_vector_type(4))) float ab_acc4;
typedef __attribute__((ext_vector_type(4))) int ab_int4;
typedef __attribute__((ext_vector_type(4))) unsigned ab_u4;

template <typename T> struct AbMfma;
template <> struct AbMfma<__hip_bfloat16> {
    static __device__ __forceinline__ ab_acc4 run(ab_frag8 a, ab_frag8 b, ab_acc4 c)
    {
        typedef __attribute__((ext_vector_type(8))) __bf16 bf8;
        return __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf8, a), __builtin_bit_cast(bf8, b), c, 0, 0, 0);
    }
};
template <> struct AbMfma<__half> {
    static __device__ __forceinline__ ab_acc4 run(ab_frag8 a, ab_frag8 b, ab_acc4 c)
    {
        typedef __attribute__((ext_vector_type(8))) _Float16 h8;
        return __builtin_amdgcn_mfma_f32_16x16x32_f16(__builtin_bit_cast(h8, a), __builtin_bit_cast(h8, b), c, 0, 0, 0);
    }
};

template <typename T> __device__ __forceinline__ short ab_round(float v)
{
    const T t = Cvt<T>::from_f(v);          // round to nearest even
    return __builtin_bit_cast(short, t);
}

// v as two 16-bit MFMA operands: hi = round(v), lo = round(v - hi).  hi + lo carries 16 (bf16) / 22 (fp16) bits of v, so
// a product accumulated over both keeps the f32 value where one rounding would leave 8 / 11 bits of it.
template <typename T> __device__ __forceinline__ void ab_split(float v, short &hi, short &lo)
{
    const T h = Cvt<T>::from_f(v);
    hi = __builtin_bit_cast(short, h);
    lo = ab_round<T>(v - Cvt<T>::to_f(h));
}

// Column `col` of rows row0 .. row0 + 7 of an f32 LDS image with `stride` bytes per row, split into hi / lo operands
template <typename T>
__device__ __forceinline__ void ab_split_column(const unsigned char *img, int row0, int stride, int col, ab_frag8 &hi, ab_frag8 &lo)
{
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        short h, l;
        ab_split<T>(*reinterpret_cast<const float *>(img + (row0 + j) * stride + col * 4), h, l);
        hi[j] = h;
        lo[j] = l;
    }
}

// Elements [row0 + j][col0 + (lane & 15)], j = 0..3 and second..second + 3, of a 16-bit LDS image with `stride` bytes per row: two
// transposed reads.  Lane 4 q + p of a 16-lane group supplies the address of row q, columns 4 p .. 4 p + 3, of the group's
// 4 x 16 block and receives the block's column (lane & 15).  Every address is 8-byte aligned (strides are multiples of
// 16, col0 of 16) and EXEC is all ones wherever this is called (wave-uniform control flow only).
__device__ __forceinline__ ab_frag8 ab_tr_pair(const unsigned char *img, int row0, int stride, int col0, int li, int second = 4)
{
    typedef __attribute__((address_space(3))) ab_frag4 lds_frag4;
    const unsigned char *p = img + (row0 + (li >> 2)) * stride + (col0 + 4 * (li & 3)) * 2;
    const ab_frag4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_frag4 *)p);
    const ab_frag4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_frag4 *)(p + second * stride));
    return ab_frag8{lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
}

struct AttnBwdArgs {
    const void *q, *k, *v, *dy;   // row r of a tensor starts at base + r * ld elements; the head adds h * HD
    void *dq, *dk, *dv;           // window form: the three thirds of dqkv; kv form: dk / dv unused (partials go to `part`)
    const float *table;           // window form: ((2 ws - 1)^2, heads) f32
    float *part;                  // kv form: f32 dK / dV partials [(problem, head)][split][2][M][HD]; window form: bin sums
                                  // [(batch, window)][heads][(2 ws - 1)^2], or NULL for no table gradient
    long q_ld, kv_ld, dy_ld;      // dq has q's row stride; window-form dk / dv have kv's
    int nq, nk;
    int heads, rpw, split;        // rounds per workgroup, workgroups per (problem, head)
    int h, w, ws, shift, nwx, nwy;
    float scale2;                 // hd^-0.5 * log2(e)
    float scale;                  // hd^-0.5
};

constexpr float kAbLog2e = 1.44269504088896340736f;
constexpr int kAbThreads = 256;

// NT2 = 32-key steps (keys padded to 32 NT2; pad keys score -inf and carry zero K / V); QW = waves (16-query tiles) of phase A
template <typename T, int HD, int NT2, bool WIN, int QW>
__global__ __launch_bounds__(kAbThreads) void attn_bwd_kernel(AttnBwdArgs a)
{
    constexpr int NK = NT2 * 32, NT = NT2 * 2, QR = 16 * QW;
    constexpr int TPW = (NT + 3) / 4;          // key tiles per wave in phase B
    constexpr int KS = HD * 2 + 16;            // bytes per K / V / Q / dO row
    constexpr int FS = NK * 4 + 16;            // bytes per f32 P / dS row
    constexpr int CH = HD / 8;                 // 16-byte chunks per head row
    constexpr int WSMAX = NT2 == 2 ? 8 : (NT2 == 5 ? 12 : 16);
    constexpr int NB = WIN ? (2 * WSMAX - 1) * (2 * WSMAX - 1) : 1;
    constexpr int NBT = (NB + kAbThreads - 1) / kAbThreads;          // bins per thread
    __shared__ __attribute__((aligned(16))) unsigned char k_lds[NK * KS];
    __shared__ __attribute__((aligned(16))) unsigned char v_lds[NK * KS];
    __shared__ __attribute__((aligned(16))) unsigned char q_lds[QR * KS];
    __shared__ __attribute__((aligned(16))) unsigned char do_lds[QR * KS];
    __shared__ __attribute__((aligned(16))) unsigned char pf_lds[QR * FS];     // P, f32, [query][key]
    __shared__ __attribute__((aligned(16))) unsigned char dsf_lds[QR * FS];    // dS, f32, [query][key]
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
        for (int n = tid; n < NK; n += kAbThreads) {
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
        for (int e = tid; e < nb; e += kAbThreads) bias_lds[e] = a.table[(long)e * a.heads + head] * kAbLog2e;
        qbase = kbase = (long)b * a.h * a.w;
        __syncthreads();
    } else {
        qbase = (long)prob * nq;
        kbase = (long)prob * nk;
    }

    const T *qp = static_cast<const T *>(a.q) + head * HD;
    const T *kp = static_cast<const T *>(a.k) + head * HD;
    const T *vp = static_cast<const T *>(a.v) + head * HD;
    const T *dyp = static_cast<const T *>(a.dy) + head * HD;
    T *dqp = static_cast<T *>(a.dq) + head * HD;

    // K and V as they lie, [key][d]; pad keys zero (0 * P = 0, never NaN)
    for (int e = tid; e < NK * CH; e += kAbThreads) {
        const int m = e / CH, c = e % CH;
        ab_u4 kk = {0u, 0u, 0u, 0u}, vv = {0u, 0u, 0u, 0u};
        if (m < nk) {
            long row = kbase;
            if constexpr (WIN) row += tok_lds[m]; else row += m;
            kk = *reinterpret_cast<const ab_u4 *>(kp + row * a.kv_ld + c * 8);
            vv = *reinterpret_cast<const ab_u4 *>(vp + row * a.kv_ld + c * 8);
        }
        *reinterpret_cast<ab_u4 *>(k_lds + m * KS + c * 16) = kk;
        *reinterpret_cast<ab_u4 *>(v_lds + m * KS + c * 16) = vv;
    }
    __syncthreads();

    const int g = lane >> 4, li = lane & 15;
    const int cst = (a.ws - 1) * (2 * a.ws - 1) + a.ws - 1;

    ab_acc4 dv[TPW][HD / 16], dk[TPW][HD / 16];
#pragma unroll
    for (int i = 0; i < TPW; ++i)
#pragma unroll
        for (int dt = 0; dt < HD / 16; ++dt) dv[i][dt] = dk[i][dt] = ab_acc4{0.f, 0.f, 0.f, 0.f};

    // the bins this thread owns (window form with a table gradient)
    float bin[NBT];
    int bdi[NBT], bdj[NBT];
    const bool bins = WIN && a.part != nullptr;
#pragma unroll
    for (int i = 0; i < NBT; ++i) {
        const int e = tid + i * kAbThreads, span = 2 * a.ws - 1;
        bin[i] = 0.f;
        bdi[i] = e / span - (a.ws - 1);          // e >= span^2 gives di >= ws: no key ever matches
        bdj[i] = e % span - (a.ws - 1);
    }

    for (int rr = 0; rr < a.rpw; ++rr) {
        const int q0 = (chunk * a.rpw + rr) * QR;
        if (q0 >= nq) break;                                          // workgroup-uniform
        if (wave < QW) {                                              // wave-uniform
            // -------- phase A: one 16-query tile per wave.  A tile past nq, or the rows of a ragged one, recompute the
            // last row with dO = 0: P stays finite, dP = D = dS = 0, so they add nothing in phase B and store nothing.
            int qn = q0 + wave * 16 + li;
            const bool qok = qn < nq;
            qn = qok ? qn : nq - 1;
            long qrow = qbase;
            if constexpr (WIN) qrow += tok_lds[qn]; else qrow += qn;
            const int lrow = wave * 16 + li;

            ab_frag8 qf[HD / 32], dof[HD / 32];
#pragma unroll
            for (int ks = 0; ks < HD / 32; ++ks) {
                qf[ks] = *reinterpret_cast<const ab_frag8 *>(qp + qrow * a.q_ld + ks * 32 + g * 8);
                dof[ks] = *reinterpret_cast<const ab_frag8 *>(dyp + qrow * a.dy_ld + ks * 32 + g * 8);
                if (!qok) dof[ks] = ab_frag8{0, 0, 0, 0, 0, 0, 0, 0};
                *reinterpret_cast<ab_frag8 *>(q_lds + lrow * KS + (ks * 32 + g * 8) * 2) = qf[ks];
                *reinterpret_cast<ab_frag8 *>(do_lds + lrow * KS + (ks * 32 + g * 8) * 2) = dof[ks];
            }

            ab_acc4 s[NT], dp[NT];
#pragma unroll
            for (int t = 0; t < NT; ++t) {
                ab_acc4 acc = {0.f, 0.f, 0.f, 0.f}, acd = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
                for (int ks = 0; ks < HD / 32; ++ks) {
                    const ab_frag8 kf = *reinterpret_cast<const ab_frag8 *>(k_lds + (16 * t + li) * KS + (ks * 32 + g * 8) * 2);
                    const ab_frag8 vf = *reinterpret_cast<const ab_frag8 *>(v_lds + (16 * t + li) * KS + (ks * 32 + g * 8) * 2);
                    acc = AbMfma<T>::run(kf, qf[ks], acc);
                    acd = AbMfma<T>::run(vf, dof[ks], acd);
                }
                s[t] = acc;
                dp[t] = acd;
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
                ab_int4 km = {0, 0, 0, 0};
                if constexpr (WIN) km = *reinterpret_cast<const ab_int4 *>(&meta_lds[16 * t + 4 * g]);
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    float v = s[t][r] * a.scale2;
                    if constexpr (WIN) {
                        v += bias_lds[qij - (km[r] & 0xffff)];
                        if ((km[r] >> 16) != qrid) v += -100.f * kAbLog2e;
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
            const float inv = 1.f / sum;
            float dsum = 0.f;
#pragma unroll
            for (int t = 0; t < NT; ++t)
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    s[t][r] *= inv;
                    dsum += s[t][r] * dp[t][r];
                }
            dsum += __shfl_xor(dsum, 16, 64);
            dsum += __shfl_xor(dsum, 32, 64);
#pragma unroll
            for (int t = 0; t < NT; ++t) {
#pragma unroll
                for (int r = 0; r < 4; ++r) dp[t][r] = s[t][r] * (dp[t][r] - dsum);
                *reinterpret_cast<ab_acc4 *>(pf_lds + lrow * FS + (16 * t + 4 * g) * 4) = s[t];
                *reinterpret_cast<ab_acc4 *>(dsf_lds + lrow * FS + (16 * t + 4 * g) * 4) = dp[t];
            }

            // dQ^T = K^T dS^T; k-step s2 = key tiles 2 s2 and 2 s2 + 1: element j of lane group g is key
            // 32 s2 + 16 (j >> 2) + 4 g + (j & 3), for both operands
            ab_acc4 o[HD / 16];
#pragma unroll
            for (int dt = 0; dt < HD / 16; ++dt) o[dt] = ab_acc4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int s2 = 0; s2 < NT2; ++s2) {
                ab_frag8 dh, dl;
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    short h0, l0, h1, l1;
                    ab_split<T>(dp[2 * s2][r], h0, l0);
                    ab_split<T>(dp[2 * s2 + 1][r], h1, l1);
                    dh[r] = h0, dl[r] = l0, dh[4 + r] = h1, dl[4 + r] = l1;
                }
#pragma unroll
                for (int dt = 0; dt < HD / 16; ++dt) {
                    const ab_frag8 kf = ab_tr_pair(k_lds, 32 * s2 + 4 * g, KS, 16 * dt, li, 16);
                    o[dt] = AbMfma<T>::run(kf, dl, o[dt]);
                    o[dt] = AbMfma<T>::run(kf, dh, o[dt]);
                }
            }
            if (qok) {
                T *dr = dqp + qrow * a.q_ld + 4 * g;
#pragma unroll
                for (int dt = 0; dt < HD / 16; ++dt) {
                    ab_frag4 out;
#pragma unroll
                    for (int r = 0; r < 4; ++r) out[r] = ab_round<T>(o[dt][r] * a.scale);
                    *reinterpret_cast<ab_frag4 *>(dr + 16 * dt) = out;
                }
            }
        }
        __syncthreads();

        // -------- phase B: dV += P^T dO, dK += dS^T Q for this wave's key tiles, over the QR queries of the round
#pragma unroll
        for (int i = 0; i < TPW; ++i) {
            const int t = wave + 4 * i;
            if (t < NT && 16 * t < nk) {                              // wave-uniform
#pragma unroll
                for (int s2 = 0; s2 < QR / 32; ++s2) {
                    ab_frag8 ph, pl, dh, dl;
                    ab_split_column<T>(pf_lds, 32 * s2 + 8 * g, FS, 16 * t + li, ph, pl);
                    ab_split_column<T>(dsf_lds, 32 * s2 + 8 * g, FS, 16 * t + li, dh, dl);
#pragma unroll
                    for (int dt = 0; dt < HD / 16; ++dt) {
                        const ab_frag8 bo = ab_tr_pair(do_lds, 32 * s2 + 8 * g, KS, 16 * dt, li);
                        const ab_frag8 bq = ab_tr_pair(q_lds, 32 * s2 + 8 * g, KS, 16 * dt, li);
                        dv[i][dt] = AbMfma<T>::run(pl, bo, dv[i][dt]);
                        dv[i][dt] = AbMfma<T>::run(ph, bo, dv[i][dt]);
                        dk[i][dt] = AbMfma<T>::run(dl, bq, dk[i][dt]);
                        dk[i][dt] = AbMfma<T>::run(dh, bq, dk[i][dt]);
                    }
                }
            }
        }
        if constexpr (WIN) {
            if (bins) {
                const int ws = a.ws;
                const int qend = nq - q0 < QR ? nq - q0 : QR;
                for (int ql = 0; ql < qend; ++ql) {                   // query order: the summation order of a bin
                    const int qi = (q0 + ql) / ws, qj = (q0 + ql) % ws;
                    const float *row = reinterpret_cast<const float *>(dsf_lds + ql * FS);
#pragma unroll
                    for (int i = 0; i < NBT; ++i) {
                        const int ki = qi - bdi[i], kj = qj - bdj[i];
                        if (ki >= 0 && ki < ws && kj >= 0 && kj < ws) bin[i] += row[ki * ws + kj];
                    }
                }
            }
        }
        __syncthreads();
    }

    // -------- results of phase B.  Lane (g, li) of key tile t, channel tile dt holds key 16 t + 4 g + r, channel 16 dt + li.
    if constexpr (WIN) {
        T *dkp = static_cast<T *>(a.dk) + head * HD;
        T *dvp = static_cast<T *>(a.dv) + head * HD;
#pragma unroll
        for (int i = 0; i < TPW; ++i) {
            const int t = wave + 4 * i;
            if (t >= NT) continue;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int key = 16 * t + 4 * g + r;
                if (key >= nk) continue;
                const long row = (kbase + tok_lds[key]) * a.kv_ld;
#pragma unroll
                for (int dt = 0; dt < HD / 16; ++dt) {
                    dkp[row + 16 * dt + li] = Cvt<T>::from_f(dk[i][dt][r] * a.scale);
                    dvp[row + 16 * dt + li] = Cvt<T>::from_f(dv[i][dt][r]);
                }
            }
        }
        if (bins) {
            const int nb = (2 * a.ws - 1) * (2 * a.ws - 1);
            float *out = a.part + (long)ph * nb;
#pragma unroll
            for (int i = 0; i < NBT; ++i) {
                const int e = tid + i * kAbThreads;
                if (e < nb) out[e] = bin[i];
            }
        }
    } else {
        float *pk = a.part + ((long)ph * a.split + chunk) * 2 * nk * HD;
        float *pv = pk + (long)nk * HD;
#pragma unroll
        for (int i = 0; i < TPW; ++i) {
            const int t = wave + 4 * i;
            if (t >= NT) continue;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int key = 16 * t + 4 * g + r;
                if (key >= nk) continue;
#pragma unroll
                for (int dt = 0; dt < HD / 16; ++dt) {
                    pk[key * HD + 16 * dt + li] = dk[i][dt][r];
                    pv[key * HD + 16 * dt + li] = dv[i][dt][r];
                }
            }
        }
    }
}

// dtable[e][head] = sum over (batch, window), in index order, of the per-workgroup bin sums
__global__ __launch_bounds__(256) void attn_bwd_table_reduce(const float *part, float *dtable, int problems, int heads, int nb)
{
    const int i = blockIdx.x * 256 + threadIdx.x;      // head * nb + e
    if (i >= heads * nb) return;
    const int head = i / nb, e = i % nb;
    float acc = 0.f;
    for (int p = 0; p < problems; ++p) acc += part[((long)p * heads + head) * nb + e];
    dtable[(long)e * heads + head] = acc;
}

// dkv[b][key][which][head][d] = round(scale_which * sum over chunks, in chunk order, of the f32 partials)
template <typename T>
__global__ __launch_bounds__(256) void attn_bwd_kv_reduce(const float *part, T *dkv, long total, int split, int m, int heads, int hd,
                                                          float scale)
{
    const long i = (long)blockIdx.x * 256 + threadIdx.x;   // (((problem, head) * 2 + which) * m + key) * hd + d
    if (i >= total) return;
    const int d = (int)(i % hd);
    long r = i / hd;
    const int key = (int)(r % m);
    r /= m;
    const int which = (int)(r & 1);
    const long ph = r >> 1;
    const int head = (int)(ph % heads);
    const long b = ph / heads;
    const long per = 2L * m * hd;
    const float *src = part + ph * split * per + ((long)which * m + key) * hd + d;
    float acc = 0.f;
    for (int c = 0; c < split; ++c) acc += src[c * per];
    if (which == 0) acc *= scale;
    dkv[((b * m + key) * 2 + which) * (long)heads * hd + head * hd + d] = Cvt<T>::from_f(acc);
}

template <typename T, int HD, bool WIN>
static int attn_bwd_launch_nt(AttnBwdArgs &a, long problems, hipStream_t s)
{
    const long grid = problems * a.split;
    TRAMBA_CHECK(grid > 0 && grid < (1L << 31), "attention backward: %ld workgroups exceed the grid", grid);
    const dim3 gr((unsigned)grid), bl(kAbThreads);
    if (a.nk <= 64)
        hipLaunchKernelGGL((attn_bwd_kernel<T, HD, 2, WIN, 4>), gr, bl, 0, s, a);
    else if (a.nk <= 160)
        hipLaunchKernelGGL((attn_bwd_kernel<T, HD, 5, WIN, 4>), gr, bl, 0, s, a);
    else
        hipLaunchKernelGGL((attn_bwd_kernel<T, HD, 8, WIN, 2>), gr, bl, 0, s, a);
    TRAMBA_LAUNCH_CHECK();
    return TRAMBA_OK;
}

template <bool WIN>
static int attn_bwd_launch(AttnBwdArgs &a, long problems, int hd, int dtype, hipStream_t s)
{
    a.scale = (float)(1.0 / sqrt((double)hd));
    a.scale2 = (float)((1.0 / sqrt((double)hd)) * 1.4426950408889634);
    if (dtype == TRAMBA_BF16)
        return hd == 32 ? attn_bwd_launch_nt<__hip_bfloat16, 32, WIN>(a, problems, s)
                        : attn_bwd_launch_nt<__hip_bfloat16, 64, WIN>(a, problems, s);
    return hd == 32 ? attn_bwd_launch_nt<__half, 32, WIN>(a, problems, s) : attn_bwd_launch_nt<__half, 64, WIN>(a, problems, s);
}

// queries per round: 64, or 32 at the cap (more than 160 keys), where LDS holds fewer rows beside K and V
static int attn_bwd_round(int nk) { return nk > 160 ? 32 : 64; }

// How the rounds of one kv-form (batch, head) are dealt to workgroups: a pure function of the shape, asked by the
// workspace size and by the launch alike, and independent of the batch, so that the workspace grows with the batch.  About
// 256 / heads workgroups per (batch, head): one batch item alone puts a workgroup on every compute unit (LDS admits no
// second) when it has that many rounds; one round per workgroup when it has fewer.
static void attn_bwd_kv_plan(int heads, long n, int m, int &rpw, int &split)
{
    const long rounds = (n + attn_bwd_round(m) - 1) / attn_bwd_round(m);
    long want = 256 / heads;
    want = want < 1 ? 1 : (want > rounds ? rounds : want);
    const long c = (rounds + want - 1) / want;
    rpw = (int)c;
    split = (int)((rounds + c - 1) / c);
}

static bool window_shape_ok(int batch, int h, int w, int heads, int hd, int ws)
{
    return (hd == 32 || hd == 64) && batch > 0 && h > 0 && w > 0 && heads > 0 && ws >= 1 && ws * ws <= 256 && h % ws == 0 &&
           w % ws == 0 && (long)h * w < (1L << 31);
}

}  // namespace tramba

using namespace tramba;

extern "C" size_t tramba_window_attn_bwd_work(int batch, int h, int w, int heads, int hd, int ws)
{
    if (!window_shape_ok(batch, h, w, heads, hd, ws)) return 0;
    return (size_t)batch * (h / ws) * (w / ws) * heads * (2 * ws - 1) * (2 * ws - 1) * sizeof(float);
}

extern "C" int tramba_window_attn_bwd_cl(const void *qkv, const float *table, const void *dy, void *dqkv, float *dtable,
                                         void *work, size_t work_bytes, int batch, int h, int w, int heads, int hd, int ws,
                                         int shift, int dtype, void *stream)
{
    TRAMBA_CHECK(qkv && table && dy && dqkv, "window_attn_bwd_cl: null tensor");
    TRAMBA_CHECK(dtype == TRAMBA_BF16 || dtype == TRAMBA_F16, "window_attn_bwd_cl: dtype %d is not bf16 / fp16", dtype);
    TRAMBA_CHECK(hd == 32 || hd == 64, "window_attn_bwd_cl: hd %d is not 32 or 64", hd);
    TRAMBA_CHECK(batch > 0 && h > 0 && w > 0 && heads > 0, "window_attn_bwd_cl: empty shape");
    TRAMBA_CHECK(ws >= 1 && ws * ws <= 256, "window_attn_bwd_cl: ws %d outside 1..16", ws);
    TRAMBA_CHECK(h % ws == 0 && w % ws == 0, "window_attn_bwd_cl: map %d x %d is no multiple of ws %d", h, w, ws);
    TRAMBA_CHECK(shift >= 0 && shift < ws, "window_attn_bwd_cl: shift %d outside 0..ws-1", shift);
    TRAMBA_CHECK((long)h * w < (1L << 31), "window_attn_bwd_cl: map %d x %d too large", h, w);
    TRAMBA_CHECK(aligned16(qkv) && aligned16(dy) && aligned16(dqkv), "window_attn_bwd_cl: tensors must be 16-byte aligned");
    const size_t need = dtable ? tramba_window_attn_bwd_work(batch, h, w, heads, hd, ws) : 0;
    TRAMBA_CHECK(need == 0 || (work && work_bytes >= need), "window_attn_bwd_cl: workspace of %zu bytes, need %zu", work ? work_bytes : (size_t)0,
                 need);
    hipStream_t s = (hipStream_t)stream;
    const long c = (long)heads * hd;
    const size_t es = 2;
    const int nb = (2 * ws - 1) * (2 * ws - 1);
    AttnBwdArgs a = {};
    a.q = qkv;
    a.k = static_cast<const char *>(qkv) + c * es;
    a.v = static_cast<const char *>(qkv) + 2 * c * es;
    a.dy = dy;
    a.dq = dqkv;
    a.dk = static_cast<char *>(dqkv) + c * es;
    a.dv = static_cast<char *>(dqkv) + 2 * c * es;
    a.table = table;
    a.part = dtable ? static_cast<float *>(work) : nullptr;
    a.q_ld = a.kv_ld = 3 * c;
    a.dy_ld = c;
    a.nq = a.nk = ws * ws;
    a.heads = heads;
    a.split = 1;
    a.rpw = (a.nq + attn_bwd_round(a.nk) - 1) / attn_bwd_round(a.nk);
    a.h = h, a.w = w, a.ws = ws, a.shift = shift, a.nwx = w / ws, a.nwy = h / ws;
    const long windows = (long)batch * a.nwx * a.nwy;
    TRAMBA_CHECK(windows < (1L << 31), "window_attn_bwd_cl: %ld windows", windows);
    const int rc = attn_bwd_launch<true>(a, windows * heads, hd, dtype, s);
    if (rc != TRAMBA_OK || !dtable) return rc;
    hipLaunchKernelGGL(attn_bwd_table_reduce, dim3((unsigned)((heads * nb + 255) / 256)), dim3(256), 0, s, a.part, dtable,
                       (int)windows, heads, nb);
    TRAMBA_LAUNCH_CHECK();
    return TRAMBA_OK;
}

extern "C" size_t tramba_kv_attn_bwd_work(int batch, int64_t n, int m, int heads, int hd)
{
    if (!((hd == 32 || hd == 64) && batch > 0 && heads > 0 && n >= 1 && n < (1L << 31) - 16 && m >= 1 && m <= 256)) return 0;
    int rpw, split;
    attn_bwd_kv_plan(heads, (long)n, m, rpw, split);
    return (size_t)batch * heads * split * 2 * m * hd * sizeof(float);
}

extern "C" int tramba_kv_attn_bwd_cl(const void *q, const void *kv, const void *dy, void *dq, void *dkv, void *work,
                                     size_t work_bytes, int batch, int64_t n, int m, int heads, int hd, int dtype, void *stream)
{
    TRAMBA_CHECK(q && kv && dy && dq && dkv, "kv_attn_bwd_cl: null tensor");
    TRAMBA_CHECK(dtype == TRAMBA_BF16 || dtype == TRAMBA_F16, "kv_attn_bwd_cl: dtype %d is not bf16 / fp16", dtype);
    TRAMBA_CHECK(hd == 32 || hd == 64, "kv_attn_bwd_cl: hd %d is not 32 or 64", hd);
    TRAMBA_CHECK(batch > 0 && heads > 0, "kv_attn_bwd_cl: empty shape");
    TRAMBA_CHECK(n >= 1 && n < (1L << 31) - 16, "kv_attn_bwd_cl: N %ld outside 1..2^31-17", (long)n);
    TRAMBA_CHECK(m >= 1 && m <= 256, "kv_attn_bwd_cl: M %d outside 1..256", m);
    TRAMBA_CHECK(aligned16(q) && aligned16(kv) && aligned16(dy) && aligned16(dq) && aligned16(dkv),
                 "kv_attn_bwd_cl: tensors must be 16-byte aligned");
    const size_t need = tramba_kv_attn_bwd_work(batch, n, m, heads, hd);
    TRAMBA_CHECK(work && work_bytes >= need, "kv_attn_bwd_cl: workspace of %zu bytes, need %zu", work ? work_bytes : (size_t)0, need);
    hipStream_t s = (hipStream_t)stream;
    const long c = (long)heads * hd;
    AttnBwdArgs a = {};
    a.q = q;
    a.k = kv;
    a.v = static_cast<const char *>(kv) + c * 2;
    a.dy = dy;
    a.dq = dq;
    a.part = static_cast<float *>(work);
    a.q_ld = a.dy_ld = c;
    a.kv_ld = 2 * c;
    a.nq = (int)n, a.nk = m;
    a.heads = heads;
    a.ws = 1;
    attn_bwd_kv_plan(heads, (long)n, m, a.rpw, a.split);
    const int rc = attn_bwd_launch<false>(a, (long)batch * heads, hd, dtype, s);
    if (rc != TRAMBA_OK) return rc;
    const long total = (long)batch * heads * 2 * m * hd;
    const dim3 gr((unsigned)((total + 255) / 256)), bl(256);
    const float scale = (float)(1.0 / sqrt((double)hd));
    if (dtype == TRAMBA_BF16)
        hipLaunchKernelGGL(attn_bwd_kv_reduce<__hip_bfloat16>, gr, bl, 0, s, a.part, static_cast<__hip_bfloat16 *>(dkv), total,
                           a.split, m, heads, hd, scale);
    else
        hipLaunchKernelGGL(attn_bwd_kv_reduce<__half>, gr, bl, 0, s, a.part, static_cast<__half *>(dkv), total, a.split, m, heads,
                           hd, scale);
    TRAMBA_LAUNCH_CHECK();
    return TRAMBA_OK;
}
