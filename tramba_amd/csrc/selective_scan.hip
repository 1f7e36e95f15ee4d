// Selective scan in the reference's own tensor layout (the L0 drop-in boundary).
//
// Replaces selective_scan_cuda_oflex.fwd / .bwd (call sites Models/SS2D/csms6s.py:910,
// :920-922).  Layout: u, delta, out (B, KD, L) with L contiguous; B/C (B, K, N, L).
//
// MI355X mapping.  The op is HBM-bound (8 B/element at bf16-in/fp32-out, ~10 flop): the
// design goal is full-width coalesced streams with enough waves in flight, not MFMA.
//   * one row (b, d) is owned by LPR consecutive lanes of a wave (LPR = 64, or 32/16 for
//     short rows so a wave carries 2/4 rows); a chunk is LPR*E consecutive positions and
//     each lane moves its E=8 elements with 16-byte accesses -> every wave-level load/store
//     covers contiguous 1 KiB (bf16) / 2 KiB (fp32) segments;
//   * inside a chunk: per-lane serial recurrence over E elements, then a log-step
//     wave-level scan of the (decay, state) pairs with DPP/shuffle (the recurrence
//     h = a h + b is associative under (a2 a1, a2 b1 + b2)), then the per-lane replay
//     with the now-known carry-in; the chunk carry is broadcast from the row's last lane;
//   * the next chunk's operands are fetched before the current chunk's scan so the
//     dependent carry chain never exposes HBM latency;
//   * state in fp32; softplus threshold 20 like the reference; exp via v_exp_f32.
// Chunk-end states go to `ckpt` for the backward (same chunking), which replays each chunk
// forward from its checkpoint and runs the adjoint recurrence right-to-left.
//
// d_state.  N = 1, 2, 4 run the templates below with N a compile-time constant (operand ring of B[N] / C[N]
// packs).  Every other N up to 16 runs the state-looped pair selective_scan_{fwd,bwd}_nloop_kernel further down: same
// chunking, checkpoints and layouts, u / delta (and dout) fetched once per chunk, the state index a run-time loop
// (in the forward with the B / C rows of the next state in flight under the current one).  What is per (row, state) -- the chunk
// carry, A, the adjoint carries -- lives in ONE register spread over the row's lanes (lane n of a row holds state
// n; N <= 16 <= LPR) and is read with a cross-lane broadcast, so the register count does not grow with N.
// No kernel in this file waits on another wave: there are no spin-waits, mailboxes or inter-wave dependencies, and
// every loop is bounded by nchunk, N or a constant, so none of them can hang by construction.
// The deterministic backward (template switch DET, tramba_selective_scan_bwd_det) adds two workgroup barriers per
// (chunk, state) around the in-LDS row sum that replaces the atomics: nchunk and N are uniform over the workgroup and no
// wave returns early, so every wave reaches every barrier; it still waits on nothing outside its own workgroup.
#include "common.h"

namespace tramba {

constexpr int kE = 8;        // elements per lane per chunk
constexpr int kMaxN = 4;     // d_state of the compile-time-N templates, instantiated for 1, 2, 4 (Tramba uses 1)
constexpr int kMaxDState = 16;  // d_state served in all: the others run the state-looped pair (lane n holds state n)
constexpr int kWavesPerBlock = 4;

__host__ __device__ inline int lanes_per_row(int l)
{
    const int need = (l + kE - 1) / kE;
    return need <= 16 ? 16 : (need <= 32 ? 32 : 64);
}

// DPP data movement (gfx9 family): a VALU-rate cross-lane read, no LDS crossbar round trip.
template <int CTRL, int ROW_MASK>
__device__ __forceinline__ float dpp_move(float old, float src)
{
    return __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(__builtin_bit_cast(int, old), __builtin_bit_cast(int, src),
                                                                 CTRL, ROW_MASK, 0xf, false));
}

// one step of the (decay, state) scan: lanes that receive a valid source combine, the others see the
// identity (1, 0) through the `old` operand
template <int CTRL, int ROW_MASK>
__device__ __forceinline__ void dpp_scan_step(float &a, float &h)
{
    const float ap = dpp_move<CTRL, ROW_MASK>(1.f, a);
    const float hp = dpp_move<CTRL, ROW_MASK>(0.f, h);
    h = fmaf(a, hp, h);
    a *= ap;
}

// inclusive scan over all 64 lanes: row_shr 1/2/4/8 inside the 16-lane rows, then row_bcast15 into
// rows 1 and 3, then row_bcast31 into rows 2 and 3
__device__ __forceinline__ void wave_scan_dpp(float &a, float &h)
{
    dpp_scan_step<0x111, 0xf>(a, h);
    dpp_scan_step<0x112, 0xf>(a, h);
    dpp_scan_step<0x114, 0xf>(a, h);
    dpp_scan_step<0x118, 0xf>(a, h);
    dpp_scan_step<0x142, 0xa>(a, h);
    dpp_scan_step<0x143, 0xc>(a, h);
}

// inclusive scan of (a, h) pairs over the LPR lanes that own one row
template <int LPR>
__device__ __forceinline__ void row_scan(float &a, float &h, int sub)
{
    if constexpr (LPR == 64) {
        wave_scan_dpp(a, h);
        return;
    }
#pragma unroll
    for (int o = 1; o < LPR; o <<= 1) {
        const float ap = __shfl_up(a, o, LPR);
        const float hp = __shfl_up(h, o, LPR);
        if (sub >= o) {
            h = fmaf(a, hp, h);
            a *= ap;
        }
    }
}

// softplus with the reference's threshold semantics, lean form: ln2*log2(1 + exp2(min(x,60)*log2e))
// max-ed with x (equal to "x > 20 -> x" to below fp32 resolution), 2 transcendentals.
__device__ __forceinline__ float softplus_lean(float x)
{
    const float z = __builtin_amdgcn_exp2f(fminf(x, 60.f) * 1.44269504088896f);
    return fmaxf(x, __builtin_amdgcn_logf(1.f + z) * 0.693147180559945f);
}

// VEC: L % 8 == 0 and 16-byte aligned tensors (every shape of the model) -> 16-byte accesses only.
template <typename T, typename TO, int LPR, int N, bool VEC>
__global__ __launch_bounds__(kWavesPerBlock * kWave) void selective_scan_fwd_kernel(
    const T *__restrict__ u, const T *__restrict__ delta, const float *__restrict__ A,
    const T *__restrict__ Bm, const T *__restrict__ Cm, const float *__restrict__ Dskip,
    const float *__restrict__ dbias, TO *__restrict__ out, float *__restrict__ ckpt, int rows_total,
    int kd, int K, int L, int nchunk, int softplus)
{
    constexpr bool vec_ok = VEC;
    constexpr int RPW = kWave / LPR;  // rows per wave
    const int lane = threadIdx.x & (kWave - 1);
    const int wave = blockIdx.x * kWavesPerBlock + (threadIdx.x >> 6);
    const int sub = lane % LPR;
    const long row = (long)wave * RPW + lane / LPR;
    const bool row_ok = row < rows_total;
    const long rrow = row_ok ? row : 0;
    const int b = (int)(rrow / kd), d = (int)(rrow % kd);
    const int k = d / (kd / K);

    const T *ur = u + rrow * L;
    const T *dr = delta + rrow * L;
    TO *yr = out + rrow * L;
    const T *Br = Bm + ((long)b * K + k) * N * L;
    const T *Cr = Cm + ((long)b * K + k) * N * L;

    float A2[N];  // A * log2(e): decay = exp2(dt * A2)
#pragma unroll
    for (int n = 0; n < N; ++n) A2[n] = A[(long)d * N + n] * 1.44269504088896f;
    const float bias = dbias ? dbias[d] : 0.f;
    const float skip = Dskip ? Dskip[d] : 0.f;

    float carry[N];
#pragma unroll
    for (int n = 0; n < N; ++n) carry[n] = 0.f;

    // Operand pipeline: a static ring of NS stages holding the RAW packed loads (converted on use), the
    // chunk loop unrolled by NS so stage indices are compile-time; loads are unconditional from clamped
    // offsets (masking happens in the arithmetic).  Two chunks stay in flight under the current one.
    constexpr int NS = (N == 1 && VEC) ? 3 : 2;
    struct Stage {
        Pack<T, kE> u, d, B[N], C[N];
    };
    Stage ring[NS];
    const int lmax = L >= kE ? L - kE : 0;
    auto fetch = [&](int chunk, Stage &st) {
        int l0 = (chunk < nchunk ? chunk : nchunk - 1) * (LPR * kE) + sub * kE;
        if (l0 > lmax) l0 = lmax;  // lanes past the row end re-read the tail; their results are masked
        if constexpr (VEC) {
            st.u = *reinterpret_cast<const Pack<T, kE> *>(ur + l0);
            st.d = *reinterpret_cast<const Pack<T, kE> *>(dr + l0);
#pragma unroll
            for (int n = 0; n < N; ++n) {
                st.B[n] = *reinterpret_cast<const Pack<T, kE> *>(Br + (long)n * L + l0);
                st.C[n] = *reinterpret_cast<const Pack<T, kE> *>(Cr + (long)n * L + l0);
            }
        } else {  // unaligned / ragged rows: element loads, clamped per element
            const int lb = chunk * (LPR * kE) + sub * kE;
#pragma unroll
            for (int j = 0; j < kE; ++j) {
                const int l = lb + j < L ? lb + j : L - 1;
                st.u.v[j] = ur[l];
                st.d.v[j] = dr[l];
#pragma unroll
                for (int n = 0; n < N; ++n) {
                    st.B[n].v[j] = Br[(long)n * L + l];
                    st.C[n].v[j] = Cr[(long)n * L + l];
                }
            }
        }
    };
#pragma unroll
    for (int i = 0; i < NS - 1; ++i) fetch(i, ring[i]);

    for (int c0 = 0; c0 < nchunk; c0 += NS) {
#pragma unroll
        for (int si = 0; si < NS; ++si) {
            const int chunk = c0 + si;
            if (chunk >= nchunk) break;  // wave-uniform
            fetch(chunk + NS - 1, ring[(si + NS - 1) % NS]);
            const Stage &st = ring[si];
            const int l0 = chunk * (LPR * kE) + sub * kE;
            // only the last chunk of a row can be ragged (wave-uniform test): dt = 0 is the identity (a=1, b=0)
            const bool ragged = (chunk + 1) * (LPR * kE) > L;
            float cu[kE], dt[kE];
#pragma unroll
            for (int j = 0; j < kE; ++j) {
                cu[j] = Cvt<T>::to_f(st.u.v[j]);
                const float x = Cvt<T>::to_f(st.d.v[j]) + bias;
                dt[j] = softplus ? softplus_lean(x) : x;
            }
            if (ragged) {
#pragma unroll
                for (int j = 0; j < kE; ++j)
                    if (l0 + j >= L) dt[j] = 0.f;
            }
            float y[kE];
#pragma unroll
            for (int j = 0; j < kE; ++j) y[j] = skip * cu[j];
#pragma unroll
            for (int n = 0; n < N; ++n) {
                float a[kE], bb[kE];
                float pa = 1.f, ph = 0.f;
#pragma unroll
                for (int j = 0; j < kE; ++j) {
                    a[j] = __builtin_amdgcn_exp2f(dt[j] * A2[n]);
                    bb[j] = dt[j] * (Cvt<T>::to_f(st.B[n].v[j]) * cu[j]);
                    ph = fmaf(a[j], ph, bb[j]);
                    pa *= a[j];
                }
                row_scan<LPR>(pa, ph, sub);
                // exclusive prefix for this lane, then fold in the chunk carry
                float ea, eh, la, lh;
                if constexpr (LPR == 64) {
                    ea = dpp_move<0x138, 0xf>(1.f, pa);  // wave_shr:1, lane 0 keeps the identity
                    eh = dpp_move<0x138, 0xf>(0.f, ph);
                    la = __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, pa), 63));
                    lh = __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, ph), 63));
                } else {
                    ea = __shfl_up(pa, 1, LPR);
                    eh = __shfl_up(ph, 1, LPR);
                    if (sub == 0) { ea = 1.f; eh = 0.f; }
                    la = __shfl(pa, LPR - 1, LPR);
                    lh = __shfl(ph, LPR - 1, LPR);
                }
                float h = fmaf(ea, carry[n], eh);
                // new chunk carry = inclusive prefix of the row's last lane applied to the old carry
                carry[n] = fmaf(la, carry[n], lh);
#pragma unroll
                for (int j = 0; j < kE; ++j) {
                    h = fmaf(a[j], h, bb[j]);
                    y[j] = fmaf(Cvt<T>::to_f(st.C[n].v[j]), h, y[j]);
                }
                if (ckpt && row_ok && sub == 0) ckpt[(rrow * nchunk + chunk) * N + n] = carry[n];
            }
            if (row_ok) {
                if (vec_ok) {
                    if (l0 + kE <= L) store_pack<TO, kE>(yr + l0, y);
                } else {
#pragma unroll
                    for (int j = 0; j < kE; ++j)
                        if (l0 + j < L) yr[l0 + j] = Cvt<TO>::from_f(y[j]);
                }
            }
        }
    }
}

// ------------------------------------------------------------------------------------ backward
// Adjoint of the recurrence, per state component n (N = 1, 2, 4 instantiated).  With g_l = dLoss/dh_l:
//     g_l      = C_l dout_l + a_{l+1} g_{l+1}                      (right-to-left scan)
//     d dt_l   = g_l (h_{l-1} a_l A + B_l u_l)        d u_l = dout_l D + g_l dt_l B_l
//     dB_l    += g_l dt_l u_l   dC_l += dout_l h_l    dA += g_l h_{l-1} a_l dt_l   dD += dout_l u_l
//     d delta  = d dt * sigmoid(delta + bias)  (1 beyond the softplus threshold)
// Chunks are walked last-to-first; each chunk is replayed forward from its checkpoint (row_scan)
// to recover h_{l-1}, then the adjoint runs as a mirrored wave scan.  dB/dC are shared by the
// KD/K rows of a group: they are reduced with fp32 atomics (one add per element); dA, dD and
// d delta_bias are reduced per row in registers, then one atomic per row.
template <int LPR>
__device__ __forceinline__ void row_scan_rev(float &a, float &g, int sub)
{
#pragma unroll
    for (int o = 1; o < LPR; o <<= 1) {
        const float an = __shfl_down(a, o, LPR);
        const float gn = __shfl_down(g, o, LPR);
        if (sub + o < LPR) {
            g = fmaf(a, gn, g);
            a *= an;
        }
    }
}

template <int LPR>
__device__ __forceinline__ float row_sum(float v)
{
#pragma unroll
    for (int o = LPR / 2; o > 0; o >>= 1) v += __shfl_xor(v, o, LPR);
    return v;
}

// ---- the deterministic (atomic-free) form of both backward kernels: the template switch DET.
// Launch: one workgroup per (batch b, group k, slab of kDetSlab<LPR, WPB> = WPB * 64 / LPR consecutive rows of the
// group's dper = KD/K), blockIdx.x = (b * K + k) * nslab + slab: no workgroup straddles a group or a batch.  Rows of the
// last slab past dper run every loop and barrier on the data of the group's first row with dout read as 0, so that all
// they stage is 0, and store nothing.  Per (chunk, state) every wave stages its rows' dB / dC contributions in LDS as
// the atomic form does; after a workgroup barrier the workgroup sums the staged rows in ascending row order and writes
// ONE partial row per slab with plain coalesced stores into part[slab][b][k][n][l]; a second workgroup barrier keeps the
// next state's staging from overwriting rows still being summed.  dA per (b, d, n), dD and d delta_bias per (b, d) leave
// as per-row partials with plain stores.  selective_scan_bwd_det_reduce_kernel then adds the slabs (dB, dC) and the
// batches (dA, dD, d delta_bias) in ascending order, so every output is a function of the inputs and the shape alone.
// The two barriers per (chunk, state) sit in loops bounded by nchunk and N, which are kernel arguments (uniform over the
// workgroup), and no wave leaves the kernel early: every barrier is reached by every wave, and the statement of the file
// header holds for this form too -- no spin-waits, no mailboxes, no dependency between workgroups, nothing that can hang.
constexpr int kDetWaves = 8;  // waves per workgroup of the deterministic form: measured against 4, faster
                               // at every N and half the slabs, i.e. half the workspace
template <int LPR, int WPB> constexpr int kDetSlab = WPB * (kWave / LPR);

// (b, group, row) of this lane in the deterministic launch; `nslab` slabs per group.  row_ok = false: past the group's end.
struct DetRow {
    int b, k, d, slab;
    bool row_ok;
};
template <int LPR, int WPB>
__device__ __forceinline__ DetRow det_row(int kd, int K, int nslab)
{
    DetRow r;
    const int dper = kd / K;
    const int grp = blockIdx.x / nslab;
    r.slab = blockIdx.x % nslab;
    r.b = grp / K;
    r.k = grp % K;
    const int lane = threadIdx.x & (kWave - 1);
    const int rg = r.slab * kDetSlab<LPR, WPB> + (threadIdx.x >> 6) * (kWave / LPR) + lane / LPR;
    r.row_ok = rg < dper;
    r.d = r.k * dper + (r.row_ok ? rg : 0);
    return r;
}

// The workgroup's staged dB / dC rows of one (chunk, state), summed in ascending row order, to the slab's partial row.
// tr[wave][0 = dB, 1 = dC][row of the wave * LPR * kE + position]; consecutive threads take consecutive positions (LDS
// bank-conflict free, 256-byte global stores per wave).  Call between two __syncthreads().
template <int LPR, int WPB>
__device__ __forceinline__ void det_slab_store(const float (*tr)[2][kWave * kE], float *__restrict__ pB,
                                               float *__restrict__ pC, int chunk, int L)
{
    constexpr int P = LPR * kE;  // positions of a chunk
    constexpr int RPW = kWave / LPR;
#pragma unroll
    for (int e = threadIdx.x; e < 2 * P; e += WPB * kWave) {
        const int t = e / P, p = e % P;
        float s = tr[0][t][p];
#pragma unroll
        for (int r = 1; r < WPB * RPW; ++r) s += tr[r / RPW][t][(r % RPW) * P + p];
        const int l = chunk * P + p;
        if (l < L) (t ? pC : pB)[l] = s;
    }
}

// DET = false: the atomic form (the default).  DET = true: the deterministic form above; then `ncopy` is the number of
// slabs per group, `copy_stride` the floats between two slabs' partials, dB / dC point at part[0], dA at the per-row
// partials (B, KD, N), dD / ddbias at (B, KD), and rows_total is unused.
template <typename T, int LPR, int N, bool DET = false, int WPB = kWavesPerBlock>
__global__ __launch_bounds__(WPB * kWave) void selective_scan_bwd_kernel(
    const T *__restrict__ u, const T *__restrict__ delta, const float *__restrict__ A,
    const T *__restrict__ Bm, const T *__restrict__ Cm, const float *__restrict__ Dskip,
    const float *__restrict__ dbias, const float *__restrict__ dout, const float *__restrict__ ckpt,
    T *__restrict__ du, T *__restrict__ ddelta, float *__restrict__ dA, float *__restrict__ dB,
    float *__restrict__ dC, float *__restrict__ dD, float *__restrict__ ddbias, int rows_total, int kd,
    int K, int L, int nchunk, int softplus, int vec_ok, int ncopy, long copy_stride)
{
    // N state components per row (d_state): the recurrences are independent, the gradients of u and delta sum over them;
    // B, C (B, K, N, L), A (KD, N), the forward's checkpoints (rows, nchunk, N).
    constexpr int RPW = kWave / LPR;
    const int lane = threadIdx.x & (kWave - 1);
    const int wave = blockIdx.x * WPB + (threadIdx.x >> 6);
    const int sub = lane % LPR;
    const long row = (long)wave * RPW + lane / LPR;
    const DetRow dr_ = DET ? det_row<LPR, WPB>(kd, K, ncopy) : DetRow{};
    const bool row_ok = DET ? dr_.row_ok : row < rows_total;
    const long rrow = DET ? (long)dr_.b * kd + dr_.d : (row_ok ? row : 0);
    const int b = DET ? dr_.b : (int)(rrow / kd), d = DET ? dr_.d : (int)(rrow % kd);
    const int k = DET ? dr_.k : d / (kd / K);

    const T *ur = u + rrow * L;
    const T *dr = delta + rrow * L;
    const float *gr = dout + rrow * L;
    const long bc = ((long)b * K + k) * N * L;
    const T *Br = Bm + bc;
    const T *Cr = Cm + bc;
    // dB/dC are shared by the KD/K rows of a group: spread the adds over `ncopy` private copies
    // (summed by the caller) so that KD/K/ncopy, not KD/K, rows contend for one address
    // (DET: the slab's partial)
    const long pc = (long)(DET ? dr_.slab : d % ncopy) * copy_stride;
    float An[N];
#pragma unroll
    for (int n = 0; n < N; ++n) An[n] = A[(long)d * N + n];
    const float bias = dbias ? dbias[d] : 0.f;
    const float skip = Dskip ? Dskip[d] : 0.f;

    // dB/dC contributions leave through LDS so that every atomic wave-instruction adds 64 CONSECUTIVE
    // floats (256 contiguous bytes): in registers lane i holds elements 8i..8i+7, which as atomics would be
    // 64 scattered 4-byte adds per instruction (an order of magnitude slower, MI355X global float atomics)
    __shared__ float tr[WPB][2][kWave * kE];
    float *trB = tr[threadIdx.x >> 6][0], *trC = tr[threadIdx.x >> 6][1];

    float g_carry[N], a_carry[N], accA[N];   // g / a of the first element of the chunk to the right, per component
#pragma unroll
    for (int n = 0; n < N; ++n) {
        g_carry[n] = 0.f;
        a_carry[n] = 1.f;
        accA[n] = 0.f;
    }
    float accD = 0.f, accBias = 0.f;

    for (int chunk = nchunk - 1; chunk >= 0; --chunk) {
        const int l0 = chunk * (LPR * kE) + sub * kE;
        float cu[kE], cd[kE], go[kE];
        if (vec_ok && l0 + kE <= L) {
            load_pack<T, kE>(ur + l0, cu);
            load_pack<T, kE>(dr + l0, cd);
            load_pack<float, kE>(gr + l0, go);
        } else {
#pragma unroll
            for (int j = 0; j < kE; ++j) {
                const bool ok = l0 + j < L;
                cu[j] = ok ? Cvt<T>::to_f(ur[l0 + j]) : 0.f;
                cd[j] = ok ? Cvt<T>::to_f(dr[l0 + j]) : 0.f;
                go[j] = ok ? gr[l0 + j] : 0.f;
            }
        }
        if constexpr (DET) {  // a row past the group's end: dout = 0, so g = 0 and everything it stages is 0
            if (!row_ok) {
#pragma unroll
                for (int j = 0; j < kE; ++j) go[j] = 0.f;
            }
        }
        float dt[kE], raw[kE], odu[kE], ddt[kE];
#pragma unroll
        for (int j = 0; j < kE; ++j) {
            raw[j] = cd[j] + bias;
            dt[j] = softplus ? softplus20(raw[j]) : raw[j];
            if (l0 + j >= L) dt[j] = 0.f;
            odu[j] = go[j] * skip;
            ddt[j] = 0.f;
            accD = fmaf(go[j], cu[j], accD);
        }
#pragma unroll
        for (int n = 0; n < N; ++n) {
            float cB[kE], cC[kE];
            if (vec_ok && l0 + kE <= L) {
                load_pack<T, kE>(Br + (long)n * L + l0, cB);
                load_pack<T, kE>(Cr + (long)n * L + l0, cC);
            } else {
#pragma unroll
                for (int j = 0; j < kE; ++j) {
                    const bool ok = l0 + j < L;
                    cB[j] = ok ? Cvt<T>::to_f(Br[(long)n * L + l0 + j]) : 0.f;
                    cC[j] = ok ? Cvt<T>::to_f(Cr[(long)n * L + l0 + j]) : 0.f;
                }
            }
            float a[kE], bb[kE];
            float pa = 1.f, ph = 0.f;
#pragma unroll
            for (int j = 0; j < kE; ++j) {
                a[j] = __expf(dt[j] * An[n]);
                bb[j] = dt[j] * cB[j] * cu[j];
                ph = fmaf(a[j], ph, bb[j]);
                pa *= a[j];
            }
            // forward replay from the checkpoint: state entering this lane
            row_scan<LPR>(pa, ph, sub);
            float ea = __shfl_up(pa, 1, LPR), eh = __shfl_up(ph, 1, LPR);
            if (sub == 0) { ea = 1.f; eh = 0.f; }
            const float hstart = chunk > 0 ? ckpt[(rrow * nchunk + chunk - 1) * N + n] : 0.f;
            float h = fmaf(ea, hstart, eh);
            float hprev[kE], hcur[kE];
#pragma unroll
            for (int j = 0; j < kE; ++j) {
                hprev[j] = h;
                h = fmaf(a[j], h, bb[j]);
                hcur[j] = h;
            }
            // adjoint scan: element j carries (a_{j+1}, C_j dout_j)
            float a_right = __shfl_down(a[0], 1, LPR);          // first a of the lane to the right
            if (sub == LPR - 1) a_right = a_carry[n];
            float an[kE], cg[kE];
#pragma unroll
            for (int j = 0; j < kE; ++j) {
                an[j] = j + 1 < kE ? a[j + 1] : a_right;
                cg[j] = cC[j] * go[j];
            }
            float qa = 1.f, qg = 0.f;
#pragma unroll
            for (int j = kE - 1; j >= 0; --j) {
                qg = fmaf(an[j], qg, cg[j]);
                qa *= an[j];
            }
            row_scan_rev<LPR>(qa, qg, sub);
            float xa = __shfl_down(qa, 1, LPR), xg = __shfl_down(qg, 1, LPR);   // exclusive suffix
            if (sub == LPR - 1) { xa = 1.f; xg = 0.f; }
            float g = fmaf(xa, g_carry[n], xg);
            // carries for the chunk to the left: full-row suffix applied to the old carry
            const float fa = __shfl(qa, 0, LPR), fg = __shfl(qg, 0, LPR);
            g_carry[n] = fmaf(fa, g_carry[n], fg);
            a_carry[n] = __shfl(a[0], 0, LPR);

#pragma unroll
            for (int j = kE - 1; j >= 0; --j) {
                g = fmaf(an[j], g, cg[j]);                       // g_j
                const bool ok = l0 + j < L;
                ddt[j] = fmaf(g, fmaf(hprev[j] * a[j], An[n], cB[j] * cu[j]), ddt[j]);
                odu[j] = fmaf(g * dt[j], cB[j], odu[j]);
                accA[n] = fmaf(g * hprev[j], a[j] * dt[j], accA[n]);
                trB[lane * kE + j] = ok ? g * dt[j] * cu[j] : 0.f;
                trC[lane * kE + j] = ok ? go[j] * hcur[j] : 0.f;
            }
            if constexpr (DET) {
                __syncthreads();  // every wave's rows are staged
                det_slab_store<LPR, WPB>(tr, dB + pc + bc + (long)n * L, dC + pc + bc + (long)n * L, chunk, L);
                __syncthreads();  // ... and summed before the next state stages again
            } else {
                __builtin_amdgcn_wave_barrier();
                if (row_ok) {
                    // lane i, step j -> element (lane/LPR)*LPR*kE + j*LPR + sub of the wave's staging area, i.e.
                    // position chunk*LPR*kE + j*LPR + sub of the row: consecutive lanes, consecutive addresses
                    const int rbase = (lane / LPR) * (LPR * kE);
#pragma unroll
                    for (int j = 0; j < kE; ++j) {
                        const int e = j * LPR + sub;
                        const int l = chunk * (LPR * kE) + e;
                        if (l < L) {
                            atomicAdd(dB + pc + bc + (long)n * L + l, trB[rbase + e]);
                            atomicAdd(dC + pc + bc + (long)n * L + l, trC[rbase + e]);
                        }
                    }
                }
                __builtin_amdgcn_wave_barrier();
            }
        }
        float odd[kE];
#pragma unroll
        for (int j = 0; j < kE; ++j) {
            float dr_ = ddt[j];
            if (softplus && raw[j] <= 20.f) dr_ = ddt[j] * sigmoidf_(raw[j]);
            odd[j] = l0 + j < L ? dr_ : 0.f;
            accBias += odd[j];
        }
        if (row_ok) {
            if (vec_ok && l0 + kE <= L) {
                store_pack<T, kE>(du + rrow * L + l0, odu);
                store_pack<T, kE>(ddelta + rrow * L + l0, odd);
            } else {
#pragma unroll
                for (int j = 0; j < kE; ++j)
                    if (l0 + j < L) {
                        du[rrow * L + l0 + j] = Cvt<T>::from_f(odu[j]);
                        ddelta[rrow * L + l0 + j] = Cvt<T>::from_f(odd[j]);
                    }
            }
        }
    }
    accD = row_sum<LPR>(accD);
    accBias = row_sum<LPR>(accBias);
#pragma unroll
    for (int n = 0; n < N; ++n) {
        const float sA = row_sum<LPR>(accA[n]);
        if (row_ok && sub == 0) {
            if constexpr (DET) dA[rrow * N + n] = sA;
            else atomicAdd(dA + (long)d * N + n, sA);
        }
    }
    if (row_ok && sub == 0) {
        if constexpr (DET) {
            if (dD) dD[rrow] = accD;
            if (ddbias) ddbias[rrow] = accBias;
        } else {
            if (dD) atomicAdd(dD + d, accD);
            if (ddbias) atomicAdd(ddbias + d, accBias);
        }
    }
}

template <typename T, typename TO, int N>
static int launch_fwd(const void *u, const void *delta, const float *A, const void *Bm, const void *Cm,
                      const float *D, const float *bias, void *out, float *ckpt, int batch, int kd,
                      int K, int L, int softplus, hipStream_t s)
{
    const int lpr = lanes_per_row(L);
    const int nchunk = (L + lpr * kE - 1) / (lpr * kE);
    const long rows = (long)batch * kd;
    const int rpw = kWave / lpr;
    const long waves = (rows + rpw - 1) / rpw;
    const long blocks = (waves + kWavesPerBlock - 1) / kWavesPerBlock;
    const int vec_ok = (L % kE == 0) && aligned16(u) && aligned16(delta) && aligned16(Bm) &&
                       aligned16(Cm) && aligned16(out);
    dim3 grid((unsigned)blocks), block(kWavesPerBlock * kWave);
#define LAUNCH_(LPR_, VEC_)                                                                             \
    hipLaunchKernelGGL((selective_scan_fwd_kernel<T, TO, LPR_, N, VEC_>), grid, block, 0, s, (const T *)u, \
                       (const T *)delta, A, (const T *)Bm, (const T *)Cm, D, bias, (TO *)out, ckpt,        \
                       (int)rows, kd, K, L, nchunk, softplus)
    if (vec_ok) {
        if (lpr == 16) LAUNCH_(16, true);
        else if (lpr == 32) LAUNCH_(32, true);
        else LAUNCH_(64, true);
    } else {
        if (lpr == 16) LAUNCH_(16, false);
        else if (lpr == 32) LAUNCH_(32, false);
        else LAUNCH_(64, false);
    }
#undef LAUNCH_
    TRAMBA_LAUNCH_CHECK();
    return TRAMBA_OK;
}

// ------------------------------------------------------------------------------------ state-looped pair (N = 3, 5..16)
// Same chunking, checkpoints and layouts as the pair above; N is a kernel argument.  Per-(row, state) values are spread
// over the lanes of the row: lane `sub == n` holds state n's chunk carry (forward), A, and the adjoint carries
// (backward); row_bcast reads them.  The n loop is a plain run-time loop, so registers and code size do not grow with N.

// the value lane n of this lane's row holds (n wave-uniform)
template <int LPR>
__device__ __forceinline__ float row_bcast(float v, int n)
{
    if constexpr (LPR == 64)
        return __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, v), n));
    else
        return __shfl(v, n, LPR);
}

template <typename T> struct BCRaw {
    Pack<T, kE> B, C;
};

// B / C of (chunk, state n) for this lane, raw.  Always in bounds: the chunk is clamped to the row's first / last one;
// 16-byte path: lanes past the row end re-read the row's tail (masked on use: dt, u and dout are 0 there); scalar path:
// elements past the row end are not loaded and read as 0.
template <typename T, int LPR, bool VEC>
__device__ __forceinline__ void fetch_bc(const T *__restrict__ Br, const T *__restrict__ Cr, int chunk, int n, int sub,
                                         int L, int nchunk, BCRaw<T> &o)
{
    if (chunk < 0) chunk = 0;
    if (chunk > nchunk - 1) chunk = nchunk - 1;
    const int lb = chunk * (LPR * kE) + sub * kE;
    const T *bp = Br + (long)n * L, *cp = Cr + (long)n * L;
    if constexpr (VEC) {
        const int lmax = L >= kE ? L - kE : 0;
        const int l0 = lb > lmax ? lmax : lb;
        o.B = *reinterpret_cast<const Pack<T, kE> *>(bp + l0);
        o.C = *reinterpret_cast<const Pack<T, kE> *>(cp + l0);
    } else {
        const T zero = Cvt<T>::from_f(0.f);
#pragma unroll
        for (int j = 0; j < kE; ++j) {
            const bool ok = lb + j < L;
            o.B.v[j] = ok ? bp[lb + j] : zero;
            o.C.v[j] = ok ? cp[lb + j] : zero;
        }
    }
}

template <typename T, typename TO, int LPR, bool VEC>
__global__ __launch_bounds__(kWavesPerBlock * kWave) __attribute__((amdgpu_waves_per_eu(4))) void selective_scan_fwd_nloop_kernel(
    const T *__restrict__ u, const T *__restrict__ delta, const float *__restrict__ A,
    const T *__restrict__ Bm, const T *__restrict__ Cm, const float *__restrict__ Dskip,
    const float *__restrict__ dbias, TO *__restrict__ out, float *__restrict__ ckpt, int rows_total,
    int kd, int K, int N, int L, int nchunk, int softplus)
{
    constexpr int RPW = kWave / LPR;  // rows per wave
    const int lane = threadIdx.x & (kWave - 1);
    const int wave = blockIdx.x * kWavesPerBlock + (threadIdx.x >> 6);
    const int sub = lane % LPR;
    const int row = wave * RPW + lane / LPR;  // rows_total is an int: so is every row index
    const bool row_ok = row < rows_total;
    const int rrow = row_ok ? row : 0;
    const int b = rrow / kd, d = rrow % kd;
    const int k = d / (kd / K);

    // The row's 64-bit offsets are formed where they are used, from two ints the compiler may not look through: formed
    // here, the per-lane pointers derived from them would all be live across the chunk loop (and spilled).
    const int row_i = rrow, group_i = b * K + k;
    auto offsets = [&](long &ro, long &bc, int &ri) {
        ri = row_i;
        int gi = group_i;
        asm volatile("" : "+v"(ri), "+v"(gi));
        ro = (long)ri * L;
        bc = (long)gi * N * L;
    };

    // lane n of the row: A[d, n] * log2(e) (decay = exp2(dt * A2)) and the chunk carry of state n
    const float A2v = sub < N ? A[(long)d * N + sub] * 1.44269504088896f : 0.f;
    float carry = 0.f;
    const float bias = dbias ? dbias[d] : 0.f;
    const float skip = Dskip ? Dskip[d] : 0.f;

    // u / delta: the two-stage raw ring of the kernel above (converted on use), the chunk loop unrolled by 2
    struct Stage {
        Pack<T, kE> u, d;
    };
    Stage ring[2];
    const int lmax = L >= kE ? L - kE : 0;
    auto fetch = [&](long ro, int chunk, Stage &st) {
        const T *ur = u + ro, *dr = delta + ro;
        const int cc = chunk < nchunk ? chunk : nchunk - 1;
        if constexpr (VEC) {
            int l0 = cc * (LPR * kE) + sub * kE;
            if (l0 > lmax) l0 = lmax;  // lanes past the row end re-read the tail; their results are masked
            st.u = *reinterpret_cast<const Pack<T, kE> *>(ur + l0);
            st.d = *reinterpret_cast<const Pack<T, kE> *>(dr + l0);
        } else {
            const int lb = cc * (LPR * kE) + sub * kE;
#pragma unroll
            for (int j = 0; j < kE; ++j) {
                const int l = lb + j < L ? lb + j : L - 1;
                st.u.v[j] = ur[l];
                st.d.v[j] = dr[l];
            }
        }
    };
    BCRaw<T> nxt;  // B / C of the state the loop computes next: one state ahead, across the chunk boundary too
    {
        long ro, bc;
        int ri;
        offsets(ro, bc, ri);
        fetch(ro, 0, ring[0]);
        fetch_bc<T, LPR, VEC>(Bm + bc, Cm + bc, 0, 0, sub, L, nchunk, nxt);
    }

    for (int c0 = 0; c0 < nchunk; c0 += 2) {
#pragma unroll
        for (int si = 0; si < 2; ++si) {
            const int chunk = c0 + si;
            if (chunk >= nchunk) break;  // wave-uniform
            long ro, bc;
            int ri;
            offsets(ro, bc, ri);
            const T *Br = Bm + bc, *Cr = Cm + bc;
            TO *yr = out + ro;
            fetch(ro, chunk + 1, ring[si ^ 1]);
            const Stage &st = ring[si];
            const int l0 = chunk * (LPR * kE) + sub * kE;
            const bool ragged = (chunk + 1) * (LPR * kE) > L;  // wave-uniform; dt = 0 is the identity (a = 1, b = 0)
            float cu[kE], dt[kE], dtu[kE], y[kE];
#pragma unroll
            for (int j = 0; j < kE; ++j) {
                cu[j] = Cvt<T>::to_f(st.u.v[j]);
                const float x = Cvt<T>::to_f(st.d.v[j]) + bias;
                dt[j] = softplus ? softplus_lean(x) : x;
            }
            if (ragged) {
#pragma unroll
                for (int j = 0; j < kE; ++j)
                    if (l0 + j >= L) dt[j] = 0.f;
            }
#pragma unroll
            for (int j = 0; j < kE; ++j) {
                dtu[j] = dt[j] * cu[j];
                y[j] = skip * cu[j];
            }
#pragma clang loop unroll(disable)
            for (int n = 0; n < N; ++n) {
                const BCRaw<T> cur = nxt;
                const bool last = n + 1 == N;
                fetch_bc<T, LPR, VEC>(Br, Cr, last ? chunk + 1 : chunk, last ? 0 : n + 1, sub, L, nchunk, nxt);
                const float a2 = row_bcast<LPR>(A2v, n);
                const float cin = row_bcast<LPR>(carry, n);
                float a[kE], bb[kE];
                float pa = 1.f, ph = 0.f;
#pragma unroll
                for (int j = 0; j < kE; ++j) {
                    a[j] = __builtin_amdgcn_exp2f(dt[j] * a2);
                    bb[j] = dtu[j] * Cvt<T>::to_f(cur.B.v[j]);
                    ph = fmaf(a[j], ph, bb[j]);
                    pa *= a[j];
                }
                row_scan<LPR>(pa, ph, sub);
                // exclusive prefix for this lane, then fold in the chunk carry
                float ea, eh, la, lh;
                if constexpr (LPR == 64) {
                    ea = dpp_move<0x138, 0xf>(1.f, pa);  // wave_shr:1, lane 0 keeps the identity
                    eh = dpp_move<0x138, 0xf>(0.f, ph);
                    la = __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, pa), 63));
                    lh = __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, ph), 63));
                } else {
                    ea = __shfl_up(pa, 1, LPR);
                    eh = __shfl_up(ph, 1, LPR);
                    if (sub == 0) { ea = 1.f; eh = 0.f; }
                    la = __shfl(pa, LPR - 1, LPR);
                    lh = __shfl(ph, LPR - 1, LPR);
                }
                float h = fmaf(ea, cin, eh);
                // new chunk carry = inclusive prefix of the row's last lane applied to the old carry; lane n keeps it
                if (sub == n) carry = fmaf(la, cin, lh);
#pragma unroll
                for (int j = 0; j < kE; ++j) {
                    h = fmaf(a[j], h, bb[j]);
                    y[j] = fmaf(Cvt<T>::to_f(cur.C.v[j]), h, y[j]);
                }
            }
            // the chunk-end states of the row, one per lane: N consecutive floats
            if (ckpt && row_ok && sub < N) ckpt[((long)ri * nchunk + chunk) * N + sub] = carry;
            if (row_ok) {
                if constexpr (VEC) {
                    if (l0 + kE <= L) store_pack<TO, kE>(yr + l0, y);
                } else {
#pragma unroll
                    for (int j = 0; j < kE; ++j)
                        if (l0 + j < L) yr[l0 + j] = Cvt<TO>::from_f(y[j]);
                }
            }
        }
    }
}

// Backward: the adjoint of the kernel above, chunk by chunk from the right as selective_scan_bwd_kernel.  u, delta and dout
// are fetched once per chunk; per state: the forward replay from the checkpoint, the mirrored adjoint scan, the two sums
// du and d dt are made of accumulated per lane, the dB / dC contributions through the wave's LDS transpose buffer (reused
// per state) as coalesced 256-byte atomics.  dA: a row sum per state and chunk, kept by lane n; one add per row and state
// at the end, as dD and d delta_bias.
// Registers: both kernels are built for four waves per SIMD (128 VGPRs).  What the state loop does not touch is kept out
// of registers across it: the row's addresses are re-formed per chunk, u and delta are read a second time after the loop,
// and the backward's two per-position accumulators live in LDS.
// DET: the deterministic form, with the launch layout, the arguments and the two workgroup barriers per (chunk, state) of
// selective_scan_bwd_kernel<.., DET = true> (see there).
template <typename T, int LPR, bool VEC, bool DET = false, int WPB = kWavesPerBlock>
__global__ __launch_bounds__(WPB * kWave) __attribute__((amdgpu_waves_per_eu(4))) void selective_scan_bwd_nloop_kernel(
    const T *__restrict__ u, const T *__restrict__ delta, const float *__restrict__ A,
    const T *__restrict__ Bm, const T *__restrict__ Cm, const float *__restrict__ Dskip,
    const float *__restrict__ dbias, const float *__restrict__ dout, const float *__restrict__ ckpt,
    T *__restrict__ du, T *__restrict__ ddelta, float *__restrict__ dA, float *__restrict__ dB,
    float *__restrict__ dC, float *__restrict__ dD, float *__restrict__ ddbias, int rows_total, int kd,
    int K, int N, int L, int nchunk, int softplus, int ncopy, long copy_stride)
{
    constexpr int RPW = kWave / LPR;
    const int lane = threadIdx.x & (kWave - 1);
    const int wave = blockIdx.x * WPB + (threadIdx.x >> 6);
    const int sub = lane % LPR;
    const int row = wave * RPW + lane / LPR;  // rows_total is an int: so is every row index
    const DetRow dr_ = DET ? det_row<LPR, WPB>(kd, K, ncopy) : DetRow{};
    const bool row_ok = DET ? dr_.row_ok : row < rows_total;
    const int rrow = DET ? dr_.b * kd + dr_.d : (row_ok ? row : 0);
    const int b = DET ? dr_.b : rrow / kd, d = DET ? dr_.d : rrow % kd;
    const int k = DET ? dr_.k : d / (kd / K);

    // what the row's 64-bit offsets are formed from, per chunk (see there): three ints
    const int row_i = rrow, group_i = b * K + k;
    const int copy_i = DET ? dr_.slab : d % ncopy;  // this row's private dB / dC copy (DET: the slab's partial)
    const float bias = dbias ? dbias[d] : 0.f;
    const float skip = Dskip ? Dskip[d] : 0.f;

    __shared__ float tr[WPB][2][kWave * kE];
    // the two per-position sums over the states (gB, gA below): slot [.][j][thread] is read and written by its lane only,
    // consecutive lanes in consecutive banks; parked here because they are touched once per state, at the very end
    __shared__ float acc[2][kE][WPB * kWave];
    float *trB = tr[threadIdx.x >> 6][0], *trC = tr[threadIdx.x >> 6][1];
    float *gB = &acc[0][0][threadIdx.x], *gA = &acc[1][0][threadIdx.x];
    constexpr int kAcc = WPB * kWave;  // stride between a lane's slots

    // lane n of the row: A[d, n]; g / a of the first element of the chunk to the right, state n
    const float Av = sub < N ? A[(long)d * N + sub] : 0.f;
    float g_carry = 0.f, a_carry = 1.f, accA = 0.f;  // accA: lane n holds dA[d, n] summed over the row so far
    float accD = 0.f, accBias = 0.f;

    for (int chunk = nchunk - 1; chunk >= 0; --chunk) {
        const int l0 = chunk * (LPR * kE) + sub * kE;
        // The row's offsets and addresses are formed here, per chunk, from three ints the compiler may not look through:
        // hoisted out of the loop, the 64-bit per-lane offsets and pointers would be live across it (about 20 registers,
        // which it then spills).  Four 64-bit multiplies per chunk instead.
        int ri = row_i, gi = group_i, ci = copy_i;
        asm volatile("" : "+v"(ri), "+v"(gi), "+v"(ci));
        const long ro = (long)ri * L;
        const long bc = (long)gi * N * L;
        const long pc = (long)ci * copy_stride;
        const T *ur = u + ro;
        const T *dr = delta + ro;
        const float *gr = dout + ro;
        const T *Br = Bm + bc;
        const T *Cr = Cm + bc;
        // u and delta of this lane's 8 positions (0 past the row end)
        // (16-byte path: L % 8 == 0, so a lane's 8 positions are all inside the row or all outside)
        auto load_ud = [&](const T *ur, const T *dr, float (&cu)[kE], float (&cd)[kE]) {
            if constexpr (VEC) {
                const int lc = l0 + kE <= L ? l0 : 0;
                load_pack<T, kE>(ur + lc, cu);
                load_pack<T, kE>(dr + lc, cd);
                if (l0 + kE > L) {
#pragma unroll
                    for (int j = 0; j < kE; ++j) cu[j] = cd[j] = 0.f;
                }
            } else {
#pragma unroll
                for (int j = 0; j < kE; ++j) {
                    const bool ok = l0 + j < L;
                    cu[j] = ok ? Cvt<T>::to_f(ur[l0 + j]) : 0.f;
                    cd[j] = ok ? Cvt<T>::to_f(dr[l0 + j]) : 0.f;
                }
            }
        };
        float go[kE], dt[kE], dtu[kE];
        {
            float cu[kE], cd[kE];
            load_ud(ur, dr, cu, cd);
            if constexpr (VEC) {
                load_pack<float, kE>(gr + (l0 + kE <= L ? l0 : 0), go);
                if (l0 + kE > L) {
#pragma unroll
                    for (int j = 0; j < kE; ++j) go[j] = 0.f;
                }
            } else {
#pragma unroll
                for (int j = 0; j < kE; ++j) go[j] = l0 + j < L ? gr[l0 + j] : 0.f;
            }
            if constexpr (DET) {  // a row past the group's end: dout = 0, so g = 0 and everything it stages is 0
                if (!row_ok) {
#pragma unroll
                    for (int j = 0; j < kE; ++j) go[j] = 0.f;
                }
            }
#pragma unroll
            for (int j = 0; j < kE; ++j) {
                const float raw = cd[j] + bias;
                dt[j] = softplus ? softplus20(raw) : raw;
                if (l0 + j >= L) dt[j] = 0.f;
                dtu[j] = dt[j] * cu[j];
                accD = fmaf(go[j], cu[j], accD);
            }
        }
        // the state entering this chunk, lane n of the row holds state n
        const float hin = (chunk > 0 && sub < N) ? ckpt[((long)ri * nchunk + chunk - 1) * N + sub] : 0.f;
        // Summed over the states (in LDS): gB = sum_n g_n B_n and gA = sum_n g_n h_{l-1} a_l A_n, from which
        //     d u = dout D + dt gB        d dt = gA + u gB
        // so that u and the raw delta are not needed inside the state loop; they are read again after it (from cache).
        // Positions past the row end need no mask inside the loop: dout and dt (so dt u) are 0 there, and every term that
        // leaves the loop carries one of them as a factor (B / C there are in-bounds re-reads or 0, see fetch_bc).
#pragma unroll
        for (int j = 0; j < kE; ++j) gB[j * kAcc] = gA[j * kAcc] = 0.f;
#pragma clang loop unroll(disable)
        for (int n = 0; n < N; ++n) {
            BCRaw<T> cur;
            fetch_bc<T, LPR, VEC>(Br, Cr, chunk, n, sub, L, nchunk, cur);
            const float An = row_bcast<LPR>(Av, n);
            const float hstart = row_bcast<LPR>(hin, n);
            const float gc = row_bcast<LPR>(g_carry, n);
            const float ac = row_bcast<LPR>(a_carry, n);
            float cB[kE];
#pragma unroll
            for (int j = 0; j < kE; ++j) cB[j] = Cvt<T>::to_f(cur.B.v[j]);
            float a[kE];
            float pa = 1.f, ph = 0.f;
#pragma unroll
            for (int j = 0; j < kE; ++j) {
                a[j] = __expf(dt[j] * An);
                ph = fmaf(a[j], ph, dtu[j] * cB[j]);
                pa *= a[j];
            }
            // forward replay from the checkpoint: state entering this lane
            row_scan<LPR>(pa, ph, sub);
            float ea = __shfl_up(pa, 1, LPR), eh = __shfl_up(ph, 1, LPR);
            if (sub == 0) { ea = 1.f; eh = 0.f; }
            float h = fmaf(ea, hstart, eh);
            float ha[kE];  // h_{l-1} a_l
#pragma unroll
            for (int j = 0; j < kE; ++j) {
                ha[j] = h * a[j];
                h = fmaf(a[j], h, dtu[j] * cB[j]);
                trC[lane * kE + j] = go[j] * h;
            }
            // adjoint scan: element j carries (a_{j+1}, C_j dout_j)
            float cg[kE];
#pragma unroll
            for (int j = 0; j < kE; ++j) cg[j] = Cvt<T>::to_f(cur.C.v[j]) * go[j];
            float a_right = __shfl_down(a[0], 1, LPR);  // first a of the lane to the right
            if (sub == LPR - 1) a_right = ac;
            float qa = 1.f, qg = 0.f;
#pragma unroll
            for (int j = kE - 1; j >= 0; --j) {
                const float an = j + 1 < kE ? a[j + 1] : a_right;
                qg = fmaf(an, qg, cg[j]);
                qa *= an;
            }
            row_scan_rev<LPR>(qa, qg, sub);
            float xa = __shfl_down(qa, 1, LPR), xg = __shfl_down(qg, 1, LPR);  // exclusive suffix
            if (sub == LPR - 1) { xa = 1.f; xg = 0.f; }
            float g = fmaf(xa, gc, xg);
            // carries for the chunk to the left: full-row suffix applied to the old carry; lane n keeps them
            const float fa = __shfl(qa, 0, LPR), fg = __shfl(qg, 0, LPR);
            const float a_first = __shfl(a[0], 0, LPR);
            if (sub == n) {
                g_carry = fmaf(fa, gc, fg);
                a_carry = a_first;
            }
            float sA = 0.f;
#pragma unroll
            for (int j = kE - 1; j >= 0; --j) {
                const float an = j + 1 < kE ? a[j + 1] : a_right;
                g = fmaf(an, g, cg[j]);  // g_j
                const float gh = g * ha[j];
                gB[j * kAcc] = fmaf(g, cB[j], gB[j * kAcc]);
                gA[j * kAcc] = fmaf(gh, An, gA[j * kAcc]);
                sA = fmaf(gh, dt[j], sA);
                trB[lane * kE + j] = g * dtu[j];
            }
            sA = row_sum<LPR>(sA);
            if (sub == n) accA += sA;
            if constexpr (DET) {
                __syncthreads();  // every wave's rows are staged
                det_slab_store<LPR, WPB>(tr, dB + pc + bc + (long)n * L, dC + pc + bc + (long)n * L, chunk, L);
                __syncthreads();  // ... and summed before the next state stages again
            } else {
                __builtin_amdgcn_wave_barrier();
                if (row_ok) {
                    // lane i, step j -> element (lane/LPR)*LPR*kE + j*LPR + sub of the wave's staging area, i.e.
                    // position chunk*LPR*kE + j*LPR + sub of the row: consecutive lanes, consecutive addresses
                    const int rbase = (lane / LPR) * (LPR * kE) + sub;
                    const int lfirst = chunk * (LPR * kE) + sub;
                    float *pB = dB + pc + bc + (long)n * L + lfirst;  // one base each, the steps are constant offsets
                    float *pC = dC + pc + bc + (long)n * L + lfirst;
#pragma unroll
                    for (int j = 0; j < kE; ++j) {
                        if (lfirst + j * LPR < L) {
                            atomicAdd(pB + j * LPR, trB[rbase + j * LPR]);
                            atomicAdd(pC + j * LPR, trC[rbase + j * LPR]);
                        }
                    }
                }
                __builtin_amdgcn_wave_barrier();
            }
        }
        float odu[kE], odd[kE];
        {
            // read again, not kept: through an offset the compiler cannot prove equal to `ro`, or it would merge this
            // read with the one before the loop and hold its 16 registers across it
            int ri2 = row_i;
            asm volatile("" : "+v"(ri2));
            const long ro2 = (long)ri2 * L;
            float cu[kE], cd[kE];
            load_ud(u + ro2, delta + ro2, cu, cd);
#pragma unroll
            for (int j = 0; j < kE; ++j) {
                const float raw = cd[j] + bias;
                const float gb = gB[j * kAcc];
                odu[j] = fmaf(dt[j], gb, go[j] * skip);
                float dr_ = fmaf(cu[j], gb, gA[j * kAcc]);
                if (softplus && raw <= 20.f) dr_ *= sigmoidf_(raw);
                odd[j] = l0 + j < L ? dr_ : 0.f;
                accBias += odd[j];
            }
        }
        if (row_ok) {
            if constexpr (VEC) {
                if (l0 + kE <= L) {
                    store_pack<T, kE>(du + ro + l0, odu);
                    store_pack<T, kE>(ddelta + ro + l0, odd);
                }
            } else {
#pragma unroll
                for (int j = 0; j < kE; ++j)
                    if (l0 + j < L) {
                        du[ro + l0 + j] = Cvt<T>::from_f(odu[j]);
                        ddelta[ro + l0 + j] = Cvt<T>::from_f(odd[j]);
                    }
            }
        }
    }
    accD = row_sum<LPR>(accD);
    accBias = row_sum<LPR>(accBias);
    // the row's channel again, from the opaque int: kept from the prologue, d and the addresses formed from it would be
    // live (and spilled) across the whole kernel
    int ri = row_i;
    asm volatile("" : "+v"(ri));
    if constexpr (DET) {  // per-row partials, (B, KD, N) and (B, KD)
        if (row_ok && sub < N) dA[(long)ri * N + sub] = accA;
        if (row_ok && sub == 0) {
            if (dD) dD[ri] = accD;
            if (ddbias) ddbias[ri] = accBias;
        }
    } else {
        const int de = ri % kd;
        if (row_ok && sub < N) atomicAdd(dA + (long)de * N + sub, accA);
        if (row_ok && sub == 0) {
            if (dD) atomicAdd(dD + de, accD);
            if (ddbias) atomicAdd(ddbias + de, accBias);
        }
    }
}

template <typename T, typename TO>
static int launch_fwd_nloop(const void *u, const void *delta, const float *A, const void *Bm, const void *Cm,
                            const float *D, const float *bias, void *out, float *ckpt, int batch, int kd, int K, int N,
                            int L, int softplus, hipStream_t s)
{
    const int lpr = lanes_per_row(L);
    const int nchunk = (L + lpr * kE - 1) / (lpr * kE);
    const long rows = (long)batch * kd;
    const int rpw = kWave / lpr;
    const long waves = (rows + rpw - 1) / rpw;
    const long blocks = (waves + kWavesPerBlock - 1) / kWavesPerBlock;
    const int vec_ok = (L % kE == 0) && aligned16(u) && aligned16(delta) && aligned16(Bm) &&
                       aligned16(Cm) && aligned16(out);
    dim3 grid((unsigned)blocks), block(kWavesPerBlock * kWave);
#define LAUNCH_(LPR_, VEC_)                                                                                     \
    hipLaunchKernelGGL((selective_scan_fwd_nloop_kernel<T, TO, LPR_, VEC_>), grid, block, 0, s, (const T *)u,   \
                       (const T *)delta, A, (const T *)Bm, (const T *)Cm, D, bias, (TO *)out, ckpt, (int)rows,  \
                       kd, K, N, L, nchunk, softplus)
    if (vec_ok) {
        if (lpr == 16) LAUNCH_(16, true);
        else if (lpr == 32) LAUNCH_(32, true);
        else LAUNCH_(64, true);
    } else {
        if (lpr == 16) LAUNCH_(16, false);
        else if (lpr == 32) LAUNCH_(32, false);
        else LAUNCH_(64, false);
    }
#undef LAUNCH_
    TRAMBA_LAUNCH_CHECK();
    return TRAMBA_OK;
}

// ------------------------------------------------------------------------------------ deterministic backward: the sum pass
// Second launch of tramba_selective_scan_bwd_det.  Up to five independent sums, one per blockIdx.y: dst[i] = src[0][i] +
// src[1][i] + ... + src[copies - 1][i] in ascending copy order, fp32 (dB, dC over the slabs; dA, dD, d delta_bias over
// the batch).  Every element of dst is written.  16-byte accesses where count % 4 == 0 and both ends are aligned.
constexpr int kDetSums = 5;
struct DetSum {
    const float *src;  // (copies, count)
    float *dst;        // (count); NULL: nothing to do (the scan kernel wrote the output itself, or the output is absent)
    long count;
    int copies;
    int vec;  // count % 4 == 0 and src, dst 16-byte aligned (set by the host)
};
struct DetSums {
    DetSum s[kDetSums];
};

__global__ __launch_bounds__(256) void selective_scan_bwd_det_reduce_kernel(DetSums args)
{
    const DetSum s = args.s[blockIdx.y];
    if (!s.dst) return;
    const long stride = (long)gridDim.x * blockDim.x;
    const long first = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (s.vec) {
        const long count4 = s.count / 4;
        for (long i = first; i < count4; i += stride) {
            float4 acc = reinterpret_cast<const float4 *>(s.src)[i];
            for (int c = 1; c < s.copies; ++c) {
                const float4 v = reinterpret_cast<const float4 *>(s.src + (long)c * s.count)[i];
                acc.x += v.x;
                acc.y += v.y;
                acc.z += v.z;
                acc.w += v.w;
            }
            reinterpret_cast<float4 *>(s.dst)[i] = acc;
        }
    } else {
        for (long i = first; i < s.count; i += stride) {
            float acc = s.src[i];
            for (int c = 1; c < s.copies; ++c) acc += s.src[(long)c * s.count + i];
            s.dst[i] = acc;
        }
    }
}

// rows of a group one workgroup of the deterministic backward covers, and the slabs per group
static int det_slab_rows(int l) { return kDetWaves * (kWave / lanes_per_row(l)); }
static int det_nslab(int kd, int k, int l) { return (kd / k + det_slab_rows(l) - 1) / det_slab_rows(l); }

}  // namespace tramba

using namespace tramba;

extern "C" int tramba_selective_scan_nchunk(int l, int io_dtype)
{
    (void)io_dtype;
    if (l <= 0) return 0;
    const int lpr = lanes_per_row(l);
    return (l + lpr * kE - 1) / (lpr * kE);
}

extern "C" int tramba_selective_scan_fwd(const void *u, const void *delta, const float *A,
                                         const void *Bm, const void *Cm, const float *D,
                                         const float *delta_bias, void *out, float *ckpt, int batch,
                                         int kd, int k, int n, int l, int io_dtype, int out_dtype,
                                         int delta_softplus, void *stream)
{
    TRAMBA_CHECK(u && delta && A && Bm && Cm && out, "selective_scan_fwd: null tensor");
    TRAMBA_CHECK(batch > 0 && kd > 0 && k > 0 && l > 0, "selective_scan_fwd: empty shape");
    TRAMBA_CHECK(kd % k == 0, "selective_scan_fwd: KD=%d is not a multiple of K=%d", kd, k);
    TRAMBA_CHECK(n >= 1 && n <= kMaxDState, "selective_scan_fwd: d_state=%d unsupported (1..%d)", n, kMaxDState);
    TRAMBA_CHECK(out_dtype == TRAMBA_F32 || out_dtype == io_dtype,
                 "selective_scan_fwd: out dtype must be f32 (oflex) or the input dtype");
    hipStream_t s = (hipStream_t)stream;
    // algorithmic bytes at the op boundary: u, delta read + out written (+ the small B/C rows)
    const double esz = (double)dtype_size(io_dtype), osz = (double)dtype_size(out_dtype);
    ProfScope prof(TRAMBA_PROF_SCAN_BOUNDARY, s,
                   (double)batch * kd * l * (2.0 * esz + osz) + 2.0 * batch * k * n * (double)l * esz);
#define GO_(T, TO, N_) \
    return launch_fwd<T, TO, N_>(u, delta, A, Bm, Cm, D, delta_bias, out, ckpt, batch, kd, k, l, delta_softplus, s)
#define BY_N_(T, TO)                                                           \
    switch (n) {                                                               \
    case 1: GO_(T, TO, 1);                                                     \
    case 2: GO_(T, TO, 2);                                                     \
    case 4: GO_(T, TO, 4);                                                     \
    default: /* 3, 5..16: the state-looped kernel */                           \
        return launch_fwd_nloop<T, TO>(u, delta, A, Bm, Cm, D, delta_bias, out, ckpt, batch, kd, k, n, l, \
                                       delta_softplus, s);                     \
    }
    TRAMBA_DISPATCH_DTYPE(io_dtype, T, {
        if (out_dtype == TRAMBA_F32) { BY_N_(T, float) } else { BY_N_(T, T) }
    });
#undef BY_N_
#undef GO_
    return TRAMBA_OK;
}

extern "C" int tramba_selective_scan_bwd(const void *u, const void *delta, const float *A, const void *Bm,
                                         const void *Cm, const float *D, const float *delta_bias,
                                         const float *dout, const float *ckpt, void *du, void *ddelta,
                                         float *dA, float *dB, float *dC, float *dD, float *ddelta_bias,
                                         int batch, int kd, int k, int n, int l, int io_dtype,
                                         int delta_softplus, int ncopy, void *stream)
{
    TRAMBA_CHECK(u && delta && A && Bm && Cm && dout && ckpt && du && ddelta && dA && dB && dC,
                 "selective_scan_bwd: null tensor");
    TRAMBA_CHECK(batch > 0 && kd > 0 && k > 0 && l > 0, "selective_scan_bwd: empty shape");
    TRAMBA_CHECK(kd % k == 0, "selective_scan_bwd: KD=%d is not a multiple of K=%d", kd, k);
    TRAMBA_CHECK(ncopy >= 1, "selective_scan_bwd: ncopy must be >= 1");
    TRAMBA_CHECK(n >= 1 && n <= kMaxDState, "selective_scan_bwd: d_state=%d unsupported (1..%d)", n, kMaxDState);
    hipStream_t s = (hipStream_t)stream;
    const int lpr = lanes_per_row(l);
    const int nchunk = (l + lpr * kE - 1) / (lpr * kE);
    const long rows = (long)batch * kd;
    const int rpw = kWave / lpr;
    const long waves = (rows + rpw - 1) / rpw;
    const long blocks = (waves + kWavesPerBlock - 1) / kWavesPerBlock;
    const int vec_ok = (l % kE == 0) && aligned16(u) && aligned16(delta) && aligned16(Bm) && aligned16(Cm) &&
                       aligned16(dout) && aligned16(du) && aligned16(ddelta);
    dim3 grid((unsigned)blocks), block(kWavesPerBlock * kWave);
#define LAUNCH_N_(T, LPR_, N_)                                                                                    \
    hipLaunchKernelGGL((selective_scan_bwd_kernel<T, LPR_, N_>), grid, block, 0, s, (const T *)u, (const T *)delta, \
                       A, (const T *)Bm, (const T *)Cm, D, delta_bias, dout, ckpt, (T *)du, (T *)ddelta, dA, dB,    \
                       dC, dD, ddelta_bias, (int)rows, kd, k, l, nchunk, delta_softplus, vec_ok, ncopy,             \
                       (long)batch * k * n * l)
#define LAUNCH_LOOP_V_(T, LPR_, VEC_)                                                                              \
    hipLaunchKernelGGL((selective_scan_bwd_nloop_kernel<T, LPR_, VEC_>), grid, block, 0, s, (const T *)u,          \
                       (const T *)delta, A, (const T *)Bm, (const T *)Cm, D, delta_bias, dout, ckpt, (T *)du,      \
                       (T *)ddelta, dA, dB, dC, dD, ddelta_bias, (int)rows, kd, k, n, l, nchunk, delta_softplus,   \
                       ncopy, (long)batch * k * n * l)
#define LAUNCH_LOOP_(T, LPR_)                          \
    if (vec_ok) { LAUNCH_LOOP_V_(T, LPR_, true); }     \
    else { LAUNCH_LOOP_V_(T, LPR_, false); }
#define LAUNCH_(T, LPR_)                                        \
    if (n == 1) { LAUNCH_N_(T, LPR_, 1); }                      \
    else if (n == 2) { LAUNCH_N_(T, LPR_, 2); }                 \
    else if (n == 4) { LAUNCH_N_(T, LPR_, 4); }                 \
    else { LAUNCH_LOOP_(T, LPR_); }   /* 3, 5..16: the state-looped kernel */
    TRAMBA_DISPATCH_DTYPE(io_dtype, T, {
        if (lpr == 16) { LAUNCH_(T, 16) }
        else if (lpr == 32) { LAUNCH_(T, 32) }
        else { LAUNCH_(T, 64) }
    });
#undef LAUNCH_
#undef LAUNCH_LOOP_
#undef LAUNCH_LOOP_V_
#undef LAUNCH_N_
    TRAMBA_LAUNCH_CHECK();
    return TRAMBA_OK;
}

// Workspace of the deterministic backward, in floats: part_B, part_C (nslab, B, K, N, L) each, then the per-row partials
// part_A (B, KD, N), part_D (B, KD), part_bias (B, KD).
extern "C" int64_t tramba_selective_scan_bwd_det_work(int batch, int kd, int k, int n, int l, int io_dtype)
{
    TRAMBA_CHECK(batch > 0 && kd > 0 && k > 0 && l > 0, "selective_scan_bwd_det_work: empty shape");
    TRAMBA_CHECK(kd % k == 0, "selective_scan_bwd_det_work: KD=%d is not a multiple of K=%d", kd, k);
    TRAMBA_CHECK(n >= 1 && n <= kMaxDState, "selective_scan_bwd_det_work: d_state=%d unsupported (1..%d)", n, kMaxDState);
    TRAMBA_CHECK(io_dtype == TRAMBA_F32 || io_dtype == TRAMBA_F16 || io_dtype == TRAMBA_BF16,
                 "selective_scan_bwd_det_work: bad dtype %d", io_dtype);
    const int64_t bknl = (int64_t)batch * k * n * l, rows = (int64_t)batch * kd;
    return 4 * (2 * det_nslab(kd, k, l) * bknl + rows * (n + 2));
}

extern "C" int tramba_selective_scan_bwd_det(const void *u, const void *delta, const float *A, const void *Bm,
                                             const void *Cm, const float *D, const float *delta_bias,
                                             const float *dout, const float *ckpt, void *du, void *ddelta,
                                             float *dA, float *dB, float *dC, float *dD, float *ddelta_bias,
                                             void *work, size_t work_bytes, int batch, int kd, int k, int n, int l,
                                             int io_dtype, int delta_softplus, void *stream)
{
    TRAMBA_CHECK(u && delta && A && Bm && Cm && dout && ckpt && du && ddelta && dA && dB && dC && work,
                 "selective_scan_bwd_det: null tensor");
    TRAMBA_CHECK(batch > 0 && kd > 0 && k > 0 && l > 0, "selective_scan_bwd_det: empty shape");
    TRAMBA_CHECK(kd % k == 0, "selective_scan_bwd_det: KD=%d is not a multiple of K=%d", kd, k);
    TRAMBA_CHECK(n >= 1 && n <= kMaxDState, "selective_scan_bwd_det: d_state=%d unsupported (1..%d)", n, kMaxDState);
    const int64_t need = tramba_selective_scan_bwd_det_work(batch, kd, k, n, l, io_dtype);
    if (need < 0) return TRAMBA_ERR_ARG;
    TRAMBA_CHECK(work_bytes >= (size_t)need, "selective_scan_bwd_det: workspace of %zu bytes, %lld needed", work_bytes,
                 (long long)need);
    TRAMBA_CHECK(((uintptr_t)work & 3) == 0, "selective_scan_bwd_det: workspace not 4-byte aligned");
    const int nslab = det_nslab(kd, k, l);
    const long rows = (long)batch * kd, groups = (long)batch * k;
    TRAMBA_CHECK(rows <= 0x7fffffffL && groups * nslab <= 0x7fffffffL,
                 "selective_scan_bwd_det: B*KD=%ld rows exceed the launch", rows);
    hipStream_t s = (hipStream_t)stream;
    const int lpr = lanes_per_row(l);
    const int nchunk = (l + lpr * kE - 1) / (lpr * kE);
    const long bknl = groups * n * l;
    const int vec_ok = (l % kE == 0) && aligned16(u) && aligned16(delta) && aligned16(Bm) && aligned16(Cm) &&
                       aligned16(dout) && aligned16(du) && aligned16(ddelta);
    // With one slab per group the scan kernel's partial row IS dB / dC, with batch 1 its per-row partials are dA, dD and
    // d delta_bias: it writes them in place and the sum pass skips them.
    float *wf = (float *)work;
    float *partB = nslab == 1 ? dB : wf, *partC = nslab == 1 ? dC : wf + (long)nslab * bknl;
    float *wr = wf + 2L * nslab * bknl;
    float *partA = batch == 1 ? dA : wr;
    float *partD = !dD ? nullptr : (batch == 1 ? dD : wr + rows * n);
    float *partBias = !ddelta_bias ? nullptr : (batch == 1 ? ddelta_bias : wr + rows * (n + 1));
    dim3 grid((unsigned)(groups * nslab)), block(kDetWaves * kWave);
#define LAUNCH_N_(T, LPR_, N_)                                                                                      \
    hipLaunchKernelGGL((selective_scan_bwd_kernel<T, LPR_, N_, true, kDetWaves>), grid, block, 0, s,                \
                       (const T *)u, (const T *)delta, A, (const T *)Bm, (const T *)Cm, D, delta_bias, dout, ckpt,  \
                       (T *)du,                                                                                     \
                       (T *)ddelta, partA, partB, partC, partD, partBias, (int)rows, kd, k, l, nchunk,              \
                       delta_softplus, vec_ok, nslab, bknl)
#define LAUNCH_LOOP_V_(T, LPR_, VEC_)                                                                               \
    hipLaunchKernelGGL((selective_scan_bwd_nloop_kernel<T, LPR_, VEC_, true, kDetWaves>), grid, block, 0, s,        \
                       (const T *)u, (const T *)delta, A, (const T *)Bm, (const T *)Cm, D, delta_bias, dout, ckpt,  \
                       (T *)du,                                                                                     \
                       (T *)ddelta, partA, partB, partC, partD, partBias, (int)rows, kd, k, n, l, nchunk,           \
                       delta_softplus, nslab, bknl)
#define LAUNCH_LOOP_(T, LPR_)                          \
    if (vec_ok) { LAUNCH_LOOP_V_(T, LPR_, true); }     \
    else { LAUNCH_LOOP_V_(T, LPR_, false); }
#define LAUNCH_(T, LPR_)                                        \
    if (n == 1) { LAUNCH_N_(T, LPR_, 1); }                      \
    else if (n == 2) { LAUNCH_N_(T, LPR_, 2); }                 \
    else if (n == 4) { LAUNCH_N_(T, LPR_, 4); }                 \
    else { LAUNCH_LOOP_(T, LPR_); }   /* 3, 5..16: the state-looped kernel */
    TRAMBA_DISPATCH_DTYPE(io_dtype, T, {
        if (lpr == 16) { LAUNCH_(T, 16) }
        else if (lpr == 32) { LAUNCH_(T, 32) }
        else { LAUNCH_(T, 64) }
    });
#undef LAUNCH_
#undef LAUNCH_LOOP_
#undef LAUNCH_LOOP_V_
#undef LAUNCH_N_
    TRAMBA_LAUNCH_CHECK();
    if (nslab == 1 && batch == 1) return TRAMBA_OK;
    DetSums sums = {};
    long most = 0;
    auto add = [&](int i, const float *src, float *dst, long count, int copies) {
        if (!dst || src == dst) return;
        sums.s[i] = DetSum{src, dst, count, copies, count % 4 == 0 && aligned16(src) && aligned16(dst)};
        if (count > most) most = count;
    };
    add(0, partB, dB, bknl, nslab);
    add(1, partC, dC, bknl, nslab);
    add(2, partA, dA, (long)kd * n, batch);
    add(3, partD, dD, kd, batch);
    add(4, partBias, ddelta_bias, kd, batch);
    // four floats per thread on the 16-byte path; the grid-stride loop covers what 8192 workgroups do not
    long rblocks = ((most + 3) / 4 + 255) / 256;
    if (rblocks > 8192) rblocks = 8192;
    hipLaunchKernelGGL(selective_scan_bwd_det_reduce_kernel, dim3((unsigned)rblocks, kDetSums), dim3(256), 0, s, sums);
    TRAMBA_LAUNCH_CHECK();
    return TRAMBA_OK;
}

extern "C" int tramba_selective_scan_max_dstate(void) { return kMaxDState; }
