/* tramba_hip.h -- C ABI of libtramba_hip.so: the MI355X (gfx950) hot path of Tramba.
 *
 * Plain pointers and sizes only (no torch types).  Every device pointer is a HIP device
 * pointer owned by the caller; nothing is retained after the call; every launch goes onto
 * the caller's `stream` (a hipStream_t passed as void*), with no implicit synchronisation,
 * no allocation and no host<->device copy inside the call (graph-capture safe).
 * Return value: 0 on success, <0 on a rejected argument (see tramba_last_error()); the
 * library never aborts the process.
 *
 * Reference interface each entry replaces (paths relative to the mj129/Tramba tree):
 *   tramba_selective_scan_fwd   selective_scan_cuda_oflex.fwd   Models/SS2D/csms6s.py:910
 *   tramba_selective_scan_bwd   selective_scan_cuda_oflex.bwd   Models/SS2D/csms6s.py:920-922
 *   tramba_scan_table           generate_indices / generate_window_indices /
 *                               generate_dilation_indices       SpiralLine.py:27-82, Window.py:3-35,
 *                                                               Dilation.py:3-45 (+ csms6s.py:18-22)
 *   tramba_cross_scan           CrossScan*.forward (= CrossMerge*.backward)
 *                                                               csms6s.py:13-22,64-72,113-121,161-172
 *   tramba_cross_merge          CrossMerge*.forward (= CrossScan*.backward)
 *                                                               csms6s.py:34-42,83-91,132-140,188-201
 *   tramba_ss2d_scan_cl /       SS2Dv2.forward_corev2 (scan -> x_proj split -> dt_proj ->
 *   tramba_ss2d_merge_norm_cl   selective scan -> merge -> out_norm) vmamba.py:230-273,
 *                               fused, channels-last
 *   tramba_layernorm_cl         LayerNorm2d.forward             Models/modules.py:22-27
 *   tramba_shuffle_norm_cl      rearrange(...)+norm in PatchExpand / FinalPatchExpand_X4 /
 *                               FreqExpand2D                    Models/modules.py:209-218,240-249,687-696
 *   tramba_dwconv_cl            SS2D.conv2d (+SiLU)             Models/vmamba.py:283-285
 *   tramba_dw_pack              weight re-layout + DWMSMlp fold (h+dw3+dw5+dw7, vmamba.py:624)
 *   tramba_dct_split_cl         DCT2D.forward                   Models/DCT_2D.py:12-29
 *   tramba_linear_cl            Linear2d.forward (1x1 conv)     Models/modules.py:10-13
 *   tramba_window_attn_cl       WindowAttention.forward + roll / window_partition / window_reverse / shift mask
 *                                                               Models/encoder/swin_encoder.py:116-147,213-268
 *   tramba_kv_attn_cl           Attention.forward (after q / kv) Models/encoder/pvtv2_encoder.py:95-116
 *   tramba_window_attn_bwd_cl / the gradients of the two above (autograd of the same reference lines), softmax rows
 *   tramba_kv_attn_bwd_cl       recomputed from q and k, nothing saved by the forward
 *   tramba_patch_conv_cl        Attention.sr (kernel = stride)  Models/encoder/pvtv2_encoder.py:76-78,103-106
 *   tramba_patch_conv_dgrad_cl / the gradients of the one above (autograd of the same reference lines): input gradient,
 *   tramba_patch_conv_wgrad_cl  weight + bias gradient
 *   tramba_patch_embed_ln       OverlapPatchEmbed (stage 1) / PatchEmbed + their LayerNorm
 *                                                               Models/encoder/pvtv2_encoder.py:159-199, swin_encoder.py:413-450
 *   tramba_conv_affine_cl       Bottleneck conv + bn (+ shortcut, ReLU), downsample conv + bn
 *                                                               Models/encoder/resnet_encoder.py:62-110
 *   tramba_stem7_affine_relu_pool  ResNet conv1 + bn1 + relu + max_pool2d
 *                                                               Models/encoder/resnet_encoder.py:62-110
 *   tramba_conv3x3s2_cl /       patch_embed + downsample convs  Models/vmamba.py:454,481-486
 *   tramba_stem_conv_ln_gelu
 *   tramba_resize_table /       get_transform(S, 'Test'): Resize + ToTensor + Normalize
 *   tramba_frames_to_input                                      data/dataloader.py:22-39, data/custom_transforms.py
 *   tramba_logits_to_u8         F.interpolate + sigmoid * 255 -> uint8 of the saved maps
 *                                                               test_TSOD.py:61-66
 *
 * "_cl" = channels-last: activations are (B, H*W, C) row-major, C contiguous.
 */
#ifndef TRAMBA_HIP_H
#define TRAMBA_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef enum { TRAMBA_F32 = 0, TRAMBA_F16 = 1, TRAMBA_BF16 = 2 } tramba_dtype;

typedef enum {
    TRAMBA_SCAN_RASTER = 0,   /* K=4 */
    TRAMBA_SCAN_LINE = 1,     /* K=4, the Bresenham half of Helix */
    TRAMBA_SCAN_HELIX = 2,    /* K=8 = raster + line */
    TRAMBA_SCAN_WINDOW = 3,   /* K=4, param = window size (0 = default rule) */
    TRAMBA_SCAN_DILATION = 4  /* K=4, param = dilation rate (0 = 4) */
} tramba_scan_family;

typedef enum { TRAMBA_ACT_NONE = 0, TRAMBA_ACT_SILU = 1, TRAMBA_ACT_GELU = 2,
               TRAMBA_ACT_SIGMOID_GATE = 3 /* GEMM epilogue only: y = sigmoid(acc + bias) * residual */,
               TRAMBA_ACT_GELU_GRAD_MUL = 4 /* GEMM epilogue only: y = (acc + bias) * gelu'(residual) -- the input gradient
                                               of `Linear(GELU(h))` in one launch, residual = h (training path) */
             } tramba_act;

#define TRAMBA_OK 0
#define TRAMBA_ERR_ARG (-1)
#define TRAMBA_ERR_UNSUPPORTED (-2)
#define TRAMBA_ERR_HIP (-3)

/* ------------------------------------------------------------------ library */
const char *tramba_last_error(void);      /* thread-local message of the last failure */
int tramba_abi_version(void);
/* Failures a kernel can only detect on the device (today: the carry mailbox of the fused scans timing out, which leaves NaN
 * in that launch's output) raise a device error word in host-mapped memory.  No call synchronises for it: EVERY entry point
 * checks the word after its own launch and, when set, clears it and returns TRAMBA_ERR_HIP with tramba_last_error() naming
 * the cause -- i.e. the failure is reported by the next library call issued after the failing kernel has run.  This entry
 * reads (and clears) the word on demand, e.g. after the caller's own stream synchronisation: TRAMBA_OK or TRAMBA_ERR_HIP.
 * (No reference counterpart: the reference's extension reports through TORCH_CHECK on the host only, csms6s.py:857.) */
int tramba_device_error(void);
/* HIP-event timing of the kernels launched by this library (used by bench.py for the
 * roofline figure).  enable=1 brackets every launch of kernel class `which` with events on
 * the launch stream; tramba_profile_read() synchronises those events and returns the
 * number of launches, writing the summed duration in milliseconds and the summed ALGORITHMIC
 * work of those launches: bytes for the scan classes, flop (2*M*N*K) for TRAMBA_PROF_GEMM
 * (DESIGN.md states the per-kernel formula). */
int tramba_profile_enable(int which, int enable);
int tramba_profile_read(int which, double *total_ms, double *total_bytes);
/* Time only the launches of class `which` that account for at least `min_units` bytes (flops): singles out one shape
 * (e.g. the Helix 96x96 fused scan inside a model forward).  0 = every launch (default). */
int tramba_profile_min_units(int which, double min_units);
/* Kernel-variant selection for A/B timing from scripts/ and for tests that pin ONE form of a kernel against the oracle
 * (never needed for correctness: 0 = the library's own choice).  MEASUREMENT-ONLY STATE: the knobs and the profile
 * classes above are the library's only process-global mutable state (SURVEY 8(b) asks for none on the operator path):
 * nothing on the product path (tramba_amd/) ever sets a knob, every knob defaults to 0, and with all knobs at 0 a call's
 * result and kernel choice depend on its arguments alone.  Not thread-safe against concurrent launches by design: set a
 * knob, time, reset.
 * knob TRAMBA_TUNE_MERGE_FORM: 1 = one wave per pixel (deep row pipeline), 2 = streaming (several pixels per wave). */
int tramba_tune_set(int knob, int value);
int tramba_tune_get(int knob);
#define TRAMBA_TUNE_MERGE_FORM 0
#define TRAMBA_TUNE_SCAN_FORM 1      /* 1 = chained (register ring), 2 = wave-segment, 3 = chained on LDS-DMA staged operands */
#define TRAMBA_TUNE_SCAN_W 2         /* waves per sequence of the register-ring chained scan (capped by the library's own choice) */
#define TRAMBA_TUNE_GEMM_TILE 3      /* 16-bit GEMMs with K % 64 == 0 (tramba_linear_cl / _ln_cl / _dual_cl): forces one form wherever it can run,
                                        else the entry's own rule.  0 = the library's rule; 7 = 64x64 LDS-DMA tiles on 4 stages (plain
                                        entry only); 13 / 14 = the same on 2 / 3 stages; 16 / 17 = producer / consumer tiles on 3 / 4
                                        stages; 18 = the rule without the producer / consumer and weight-stationary forms (the r03
                                        kernels; it alone also reaches tramba_linear2_cl and tramba_conv3x3s2_cl: their register-staged
                                        kernels); 19 = weight-stationary wherever it can run.  Other values are refused. */
#define TRAMBA_TUNE_MAILBOX_SKIP 4   /* tests only: > 0 withholds the carry hand-over of that tile (chain order) in the fused scans, so that
                                        the wave waiting for it runs out of polls (~0.1 s) and the device error word is raised; 0 = off */
                                     /* knob 5 (the weight-gradient form) is retired: refused */
#define TRAMBA_TUNE_DW_FORM 6        /* 7x7 depth-wise stencil and its weight gradient: 1 = the r03 kernels (one output row per thread / tap row outer),
                                        0 = the kernels that march down a band of rows (default) */
#define TRAMBA_TUNE_DW_ROWS 7        /* rows per band of the marching 7x7 kernels (0 = the library's choice) */
#define TRAMBA_TUNE_MERGE_PW 8       /* pixels per wave of the streaming merge: 4 / 8 / 16 force one (0 = the library's choice, by the wave count) */
#define TRAMBA_TUNE_SCAN_N_PASS 9  /* measurement only (scripts/bench_ss2d_dstate.py): tramba_ss2d_scan_n_cl launches 1 = its reduce pass alone,
                                    * 2 = its replay pass alone (the carries are then whatever an earlier reduce pass left in the workspace) */
#define TRAMBA_TUNE_COUNT 10
#define TRAMBA_PROF_SCAN_BOUNDARY 0
#define TRAMBA_PROF_SCAN_FUSED 1
#define TRAMBA_PROF_GEMM 2          /* tramba_linear_cl (1x1-conv projections) */
#define TRAMBA_PROF_MERGE 3         /* tramba_ss2d_merge_norm_cl: K*L*D ys bytes read + L*D written, per image */
#define TRAMBA_PROF_SCAN_BWD 4      /* tramba_ss2d_scan_bwd_cl: SURVEY 8(d) backward bytes of the op it replaces, 12 B per (b,k,d,l)
                                       element at 16-bit activations (u, delta, dout read; du, ddelta written), 20 B at fp32 */
#define TRAMBA_PROF_WGRAD 5         /* tramba_wgrad_cl: 2*M*N*K flop per group and batch */
#define TRAMBA_PROF_LAYERNORM 6     /* the LayerNorm family (tramba_layernorm_cl, tramba_add_layernorm_cl, tramba_shuffle_norm_cl and the
                                       tramba_layernorm_bwd_* / tramba_shuffle_norm_bwd_cl launches): bytes of every activation-sized tensor
                                       the call reads or writes once (x, dy, dx, the residual and its sum ... ), the per-channel rows not counted */
#define TRAMBA_PROF_DW 7            /* the depth-wise stencils (tramba_dwconv_cl / _dual_cl: x read, y (and y_pre) written;
                                       tramba_dwconv_wgrad_cl: x and gy read) */
#define TRAMBA_PROF_COUNT 8

/* ------------------------------------------------------------------ scan-order tables (host) */
/* Number of directions K of a family. */
int tramba_scan_family_k(int family);
/* Default window size this library uses for feature size h (reference values for
 * 12/24/48/96, csms6s.py:107-108; documented rule otherwise). */
int tramba_default_window(int h);
/* Fills out[K*h*w] (HOST memory) with the flat pixel index (row*w+col) read at each
 * sequence position of each direction.  Returns K, or <0. */
int tramba_scan_table(int family, int h, int w, int param, int32_t *out);
/* Inverse (CSR) of a table for the deterministic merge: for pixel p,
 * entries inv_idx[inv_ptr[p] .. inv_ptr[p+1]) hold k*L+l with table[k][l]==p, ascending.
 * inv_ptr has L+1 entries, inv_idx has K*L.  HOST memory. */
int tramba_scan_table_inverse(const int32_t *table, int k, int l, int32_t *inv_ptr, int32_t *inv_idx);

/* ------------------------------------------------------------------ L0: selective scan, reference layout */
/* u, delta: (B, KD, L) io_dtype;  A: (KD, N) f32;  Bm, Cm: (B, K, N, L) io_dtype;
 * D, delta_bias: (KD) f32 or NULL;  out: (B, KD, L) out_dtype (f32 = "oflex");
 * ckpt: (B, KD, nchunk, N) f32 chunk-end states for the backward, or NULL;
 * nchunk = tramba_selective_scan_nchunk(L, io_dtype). */
int tramba_selective_scan_nchunk(int l, int io_dtype);
/* the largest d_state tramba_selective_scan_fwd / _bwd accept (16) */
int tramba_selective_scan_max_dstate(void);
int tramba_selective_scan_fwd(const void *u, const void *delta, const float *A, const void *Bm,
                              const void *Cm, const float *D, const float *delta_bias, void *out,
                              float *ckpt, int batch, int kd, int k, int n, int l, int io_dtype,
                              int out_dtype, int delta_softplus, void *stream);
/* du, ddelta: (B, KD, L) io_dtype; dA (KD,N), dD, ddelta_bias (KD): f32, ACCUMULATED into
 * (caller zeroes);  dB, dC: (ncopy, B, K, N, L) f32, accumulated into (caller zeroes) -- the rows of a
 * direction group spread their atomic adds over `ncopy` private copies which the caller sums.
 * Both directions: d_state N = 1 .. 16 (tramba_selective_scan_max_dstate()); outside that range the call returns an
 * error that names d_state and the limit.  N = 1 (everything Tramba builds), 2 and 4 run kernels with N a compile-time
 * constant; every other N runs a state-looped pair with the same chunking, checkpoints and layouts. */
int tramba_selective_scan_bwd(const void *u, const void *delta, const float *A, const void *Bm,
                              const void *Cm, const float *D, const float *delta_bias,
                              const float *dout, const float *ckpt, void *du, void *ddelta,
                              float *dA, float *dB, float *dC, float *dD, float *ddelta_bias,
                              int batch, int kd, int k, int n, int l, int io_dtype,
                              int delta_softplus, int ncopy, void *stream);
/* The deterministic (atomic-free) form of tramba_selective_scan_bwd: same inputs, same seven outputs in the same dtypes
 * and shapes -- dA (KD,N), dB, dC (B, K, N, L), dD, ddelta_bias (KD) -- every element WRITTEN (the caller zeroes nothing),
 * each a function of the inputs and the shape alone: no atomics, fixed summation order (bitwise reproducible).  First
 * launch: one workgroup per (batch, group, slab of S = 512 / LPR consecutive rows of the group's KD/K -- eight waves; LPR = 64
 * lanes per row for L > 256, 32 for L > 128, else 16, so S = 8, 16 or 32) sums its rows' dB / dC contributions in LDS in ascending row order and stores
 * one partial row per slab; dA, dD, ddelta_bias leave as per-row partials.  Second launch: dB, dC = the ascending-slab
 * sum, dA, dD, ddelta_bias = the ascending-batch sum, in f32.  The caller allocates the workspace;
 * tramba_selective_scan_bwd_det_work returns its size in bytes (negative on bad arguments),
 *     4 * (2 * ceil((KD/K) / S) * B*K*N*L + B*KD*(N + 2)),
 * i.e. per tensor at most ceil((KD/K) / 4) copies of (B, K, N, L) f32, and the entry checks work_bytes against it.  The
 * contents of the workspace on entry do not matter.  No allocation or synchronisation (capturable). */
int64_t tramba_selective_scan_bwd_det_work(int batch, int kd, int k, int n, int l, int io_dtype);
int tramba_selective_scan_bwd_det(const void *u, const void *delta, const float *A, const void *Bm,
                                  const void *Cm, const float *D, const float *delta_bias,
                                  const float *dout, const float *ckpt, void *du, void *ddelta,
                                  float *dA, float *dB, float *dC, float *dD, float *ddelta_bias,
                                  void *work, size_t work_bytes, int batch, int kd, int k, int n, int l,
                                  int io_dtype, int delta_softplus, void *stream);

/* ------------------------------------------------------------------ L1: scan-order gather / merge, NCHW */
/* xs[b,k,c,l] = x[b,c,table[k,l]];  x: (B, C, L), xs: (B, K, C, L);  table: DEVICE int32 (K, L). */
int tramba_cross_scan(const void *x, const int32_t *table, void *xs, int batch, int c, int l, int k,
                      int dtype, void *stream);
/* y[b,c,p] = sum over entries e=k*L+l of inv[p] of ys[b,k,c,l];  fp32 accumulation, fixed order. */
int tramba_cross_merge(const void *ys, const int32_t *inv_ptr, const int32_t *inv_idx, void *y,
                       int batch, int c, int l, int k, int dtype, void *stream);

/* ------------------------------------------------------------------ fused SS2D core, channels-last */
/* x:    (B, L, D)           dtype   -- conv+SiLU output, spatial order
 * xdbl: (B, L, K*RG)        f32     -- x_proj output in SPATIAL order: per group k
 *                                      [dt_0..dt_{R-1}, 0-pad to R8, B, C, 0, 0]  (d_state N = 1 only);
 *                                      R8 = R rounded up to 8, RG = tramba_ss2d_group_stride(R) = R8 + 4
 * table (K, L) int32 device; dt_w (K, D, R) f32; dt_bias (K*D) f32; A (K*D) f32 (= -exp(A_logs));
 * Ds (K*D) f32.   ys: (B, K, L, D) ys_dtype in SEQUENCE order.                                   */
int tramba_ss2d_group_stride(int r);
/* workspace (device memory, 16-byte aligned, >= tramba_ss2d_scan_workspace() bytes) selects the
 * wave-segment form: segment reduce -> carry scan -> segment replay, every wave independent.  With
 * workspace == NULL the chained single-pass kernel (one workgroup per sequence) runs instead.
 * states (training; NULL otherwise, requires ys_dtype == dtype): tramba_ss2d_scan_bwd_workspace() bytes that receive the
 * recurrence state entering every 32-position tile, (B, K, ceil(L/32) + 8, D) f32 -- handed to tramba_ss2d_scan_bwd_cl as
 * its workspace with have_states = 1, the backward skips the sweep that would recompute them.
 * a_log (training, chained forms): `A` holds the PARAMETER A_logs (K*D) and the kernel forms A = -exp(A_logs) itself
 * (vmamba.py:246) -- no exp / negation launch per block and step. */
size_t tramba_ss2d_scan_workspace(int batch, int l, int d, int k);
int tramba_ss2d_scan_cl(const void *x, const float *xdbl, const int32_t *table, const float *dt_w,
                        const float *dt_bias, const float *A, const float *Ds, void *ys, void *workspace,
                        size_t workspace_bytes, int batch, int l, int d, int k, int r, int dtype,
                        int ys_dtype, float *states, int a_log, void *stream);
/* The same scan for d_state N = 2..16 (inference; replaces vmamba.py:230-257 at the reference's default d_state = 16).
 * xdbl: (B, L, K*RG) f32, per group k [dt_0..dt_{R-1}, 0-pad to R8 | B_0..B_{N-1} | C_0..C_{N-1} | 0-pad to a multiple
 *       of 4 floats];  RG = tramba_ss2d_group_stride_n(R, N) = R8 + ((2N + 3) & ~3), which is tramba_ss2d_group_stride(R)
 *       at N = 1.
 * A (K*D, N) f32 (= -exp(A_logs)); every other tensor as for tramba_ss2d_scan_cl.  r <= 64.
 * N = 1 is an argument error here (tramba_ss2d_scan_cl serves it), as is N > 16.
 * Always the wave-segment form: one wave per segment, two launches (one when the plan has a single segment), no
 * workgroup barrier and no wait between waves.  workspace: >= tramba_ss2d_scan_n_workspace() bytes, 16-byte aligned;
 * required when the plan has more than one segment; every byte the second launch reads is written by the first.
 * tramba_ss2d_scan_n_plan: host-only query of that plan (tiles of 32 positions per segment, segments per sequence). */
int tramba_ss2d_group_stride_n(int r, int n);
size_t tramba_ss2d_scan_n_workspace(int batch, int l, int d, int k, int n);
int tramba_ss2d_scan_n_plan(int batch, int l, int d, int k, int n, int *tiles_per_segment, int *nseg);
int tramba_ss2d_scan_n_cl(const void *x, const float *xdbl, const int32_t *table, const float *dt_w,
                          const float *dt_bias, const float *A, const float *Ds, void *ys, void *workspace,
                          size_t workspace_bytes, int batch, int l, int d, int k, int r, int n, int dtype,
                          int ys_dtype, void *stream);
/* Training: backward of tramba_ss2d_scan_cl + the merge that follows it.  gym (B, L, D), f32 or dtype (gym_dtype), is the
 * gradient of the MERGED map (CrossMerge output, before out_norm); the kernel gathers it through `table`.  Outputs, in SEQUENCE
 * order like ys: gu (B,K,L,D) dtype = dL/d(gathered x) -- merge it with tramba_ss2d_merge_norm_cl(eps < 0) to get
 * dL/dx; graw (B,K,L,D) dtype = dL/d(x_proj ranks . dt_w) before bias and softplus; gB, gC (B,K,L) f32 ACCUMULATED
 * (zero them first), element (b,k,l) at gB[((b*K + k)*L + l) * bc_stride] -- bc_stride = 1 for packed arrays, or the row
 * stride of a (B,K,L,RG) x_dbl-gradient table whose B / C columns the two pointers address; gpar (B,3,K,D) f32 = per-channel dA, dD, d(dt_bias) planes (sum over B for the parameters).
 * workspace: tramba_ss2d_scan_bwd_workspace() bytes of device scratch -- or, with have_states = 1, the `states` buffer the
 * forward launch filled. */
size_t tramba_ss2d_scan_bwd_workspace(int batch, int l, int d, int k);
int tramba_ss2d_scan_bwd_cl(const void *x, const float *xdbl, const int32_t *table, const float *dt_w,
                            const float *dt_bias, const float *A, const float *Ds, const void *gym, void *gu,
                            void *graw, float *gB, float *gC, int bc_stride, float *gpar, void *workspace,
                            size_t workspace_bytes, int have_states, int batch, int l, int d, int k, int r, int dtype,
                            int gym_dtype, int flags, void *stream);
/* flags of tramba_ss2d_scan_bwd_cl:
 *   1  `A` holds A_logs (as a_log of the forward) and gpar's first plane is dL/dA_logs (= dL/dA * A)
 *   2  gB / gC are (B, K, ceil(D/32), L) f32 tables of per-channel-tile partial sums, every element written by exactly one
 *      wave: no zero fill and no atomics (reproducible); tramba_ss2d_bwd_prep_cl adds the partials in a fixed order.
 *      bc_stride is ignored. */
#define TRAMBA_SCAN_BWD_A_LOG 1
#define TRAMBA_SCAN_BWD_BC_PARTIALS 2
/* Training, after tramba_ss2d_scan_bwd_cl(flags & 2), r = dt_rank, R8 = 8*ceil(r/8), RG = R8 + 4:
 *   ranks (B, K, L, R8) dtype = xdbl[b, table[k][i], k*RG .. k*RG + R8): the dt-rank rows in SEQUENCE order, the operand of
 *         the dt_projs_weight gradient (tramba_wgrad_cl with groups = K);
 *   gseq  (B, K, L, RG) f32: columns R8, R8 + 1 = dL/dB, dL/dC summed over the channel tiles (fixed order), R8 + 2, R8 + 3 = 0;
 *         the rank columns 0 .. r are written afterwards by tramba_rows_gemm_cl(graw, dt_projs_weight^T, ldy = RG). */
int tramba_ss2d_bwd_prep_cl(const float *xdbl, const int32_t *table, const float *bpart, const float *cpart, void *ranks,
                            float *gseq, int batch, int l, int k, int r, int ctiles, int dtype, void *stream);
/* out (B, L, K*RG) dtype = the x_dbl-row gradients of gseq (B, K, L, RG) f32 brought back from sequence to spatial order:
 * out[b, p, k*RG + j] = sum over the entries (k, i) of pixel p in the inverse table of gseq[b, k, i, j] for j < r and
 * j in {R8, R8 + 1}, 0 elsewhere -- a gather-sum in CSR order (deterministic; the Helix lines revisit pixels), the adjoint of
 * the scan kernels' gather of x_dbl rows, cast to the dtype the x_proj gradient GEMMs read. */
int tramba_ss2d_bwd_assemble_cl(const float *gseq, const int32_t *inv_ptr, const int32_t *inv_idx, void *out, int batch,
                                int l, int k, int r, int dtype, void *stream);
/* Training at d_state N = 2..16: backward of tramba_ss2d_scan_n_cl + the merge that follows it (replaces vmamba.py:230-262
 * under autograd, i.e. csms6s.py selective_scan_cuda_oflex.bwd with the gathers, dt_proj and the merge around it).
 * x, xdbl (layout of tramba_ss2d_scan_n_cl), table, dt_w, dt_bias, A (K*D, N) f32 = -exp(A_logs), Ds, gym as for
 * tramba_ss2d_scan_bwd_cl.  Outputs, every element written by exactly one wave (no zero fill, no atomics, bitwise
 * reproducible):
 *   gu, graw (B,K,L,D) dtype, in sequence order;
 *   bpart, cpart (B, K, ceil(D/32), N, L) f32: per-channel-tile partial sums of dL/dB_n, dL/dC_n
 *         (tramba_ss2d_bwd_prep_n_cl adds them in a fixed order);
 *   gpar  (B * NSEG, K*D*(N + 2)) f32, NSEG from tramba_ss2d_scan_n_bwd_plan: one slab per (batch, segment) holding
 *         [dL/dA_logs (K*D, N) = dL/dA * A | dD (K*D) | d(dt_bias) (K*D)]; the sum over the slabs (tramba_slab_sum) has the
 *         parameters' own strides.
 * Wave-segment form only: one wave per segment of a (b, k, 32-channel tile); three launches (ss2d_seg_n_kernel's reduce
 * pass, an adjoint reduce pass, the emit pass), one when the plan has a single segment; no workgroup barrier, no wait
 * between waves.  The plan is the backward's own: segments of at most 160 / N tiles, whose tile-entry states stay in LDS.
 * workspace: launch-local scratch, >= tramba_ss2d_scan_n_bwd_workspace() bytes, 16-byte aligned, required when NSEG > 1:
 *   bytes = 16 if NSEG == 1, else B*K*NSEG*N*D * 12  (the forward (decay, state) float2 pairs, then the adjoint floats);
 *   0 for arguments outside the supported range.  Every byte read is written earlier in the same call.
 * tramba_ss2d_scan_n_bwd_plan: host-only query (tiles of 32 positions per segment, segments per sequence). */
size_t tramba_ss2d_scan_n_bwd_workspace(int batch, int l, int d, int k, int n, int dtype);
int tramba_ss2d_scan_n_bwd_plan(int batch, int l, int d, int k, int n, int *tiles_per_segment, int *nseg);
int tramba_ss2d_scan_n_bwd_cl(const void *x, const float *xdbl, const int32_t *table, const float *dt_w,
                              const float *dt_bias, const float *A, const float *Ds, const void *gym, void *gu,
                              void *graw, float *bpart, float *cpart, float *gpar, void *workspace,
                              size_t workspace_bytes, int batch, int l, int d, int k, int r, int n, int dtype,
                              int gym_dtype, void *stream);
/* The glue of tramba_ss2d_bwd_prep_cl / tramba_ss2d_bwd_assemble_cl for d_state n = 1..16, RG = tramba_ss2d_group_stride_n(r, n)
 * (n = 1: exactly the two entries above): bpart / cpart (B, K, CT, n, L); gseq columns R8 .. R8 + n - 1 = dL/dB_0..,
 * R8 + n .. R8 + 2n - 1 = dL/dC_0.., the pad columns 0; the assemble keeps columns j < r and R8 <= j < R8 + 2n.
 * RG <= 96 (r <= 64, n <= 16). */
int tramba_ss2d_bwd_prep_n_cl(const float *xdbl, const int32_t *table, const float *bpart, const float *cpart, void *ranks,
                              float *gseq, int batch, int l, int k, int r, int n, int ctiles, int dtype, void *stream);
int tramba_ss2d_bwd_assemble_n_cl(const float *gseq, const int32_t *inv_ptr, const int32_t *inv_idx, void *out, int batch,
                                  int l, int k, int r, int n, int dtype, void *stream);
/* y[b,p,:] = act(LayerNorm_D(sum_{e in inv[p]} ys[b, e/L, e%L, :]));  y: (B, L, D) dtype.
 * eps < 0: the plain sum (CrossMerge alone), ln_w / ln_b / act ignored. */
int tramba_ss2d_merge_norm_cl(const void *ys, const int32_t *inv_ptr, const int32_t *inv_idx,
                              const float *ln_w, const float *ln_b, void *y, int batch, int l, int d,
                              int k, float eps, int act, int ys_dtype, int dtype, void *stream);
/* The same merge with the epilogue of SS2D's input gradient (training; eps < 0 only): y = (sum + addend) * silu'(zpre),
 * addend (B, L, D) dtype or NULL = the x_proj branch's gradient, zpre (B, L, D) dtype = the pre-activation of the SiLU in front
 * of the core (vmamba.py:283-285). */
int tramba_ss2d_merge_grad_cl(const void *ys, const int32_t *inv_ptr, const int32_t *inv_idx, const float *ln_w,
                              const float *ln_b, void *y, const void *addend, const void *zpre, int batch, int l, int d,
                              int k, float eps, int act, int ys_dtype, int dtype, void *stream);
/* tramba_ss2d_merge_norm_cl with SS2D's z gate (vmamba.py:288-290) in the epilogue: y = act(LayerNorm(merge(ys))) * silu(zpre),
 * zpre (B, L, D) dtype, 16-byte aligned = the gate's PRE-activation (the z half of in_proj as the GEMM wrote it; the silu is
 * evaluated in fp32 here).  eps >= 0 only: a merge-only call has no gate.  The kernel form chosen for a shape is that of the
 * ungated entry, and so are the sums, the statistics and their order. */
int tramba_ss2d_merge_norm_gate_cl(const void *ys, const int32_t *inv_ptr, const int32_t *inv_idx, const float *ln_w,
                                   const float *ln_b, const void *zpre, void *y, int batch, int l, int d, int k, float eps,
                                   int act, int ys_dtype, int dtype, void *stream);

/* ------------------------------------------------------------------ element / stencil kernels, channels-last */
/* y = act(LayerNorm_C(x));  x, y: (rows, C).  w, b f32. */
int tramba_layernorm_cl(const void *x, const float *w, const float *b, void *y, int64_t rows, int c,
                        float eps, int act, int dtype, void *stream);
/* Training: LayerNorm backward over the last dim of (rows, C): dx in dtype; part (P, 2, C) f32 receives P partial
 * (dgamma, dbeta) rows (one per wave, or per workgroup for short rows), P = tramba_layernorm_bwd_parts(rows, c, dtype): the
 * caller sums over P (tramba_slab_sum: fixed order -> reproducible).  mean / rstd are recomputed from x. */
int64_t tramba_layernorm_bwd_parts(int64_t rows, int c, int dtype);
int tramba_layernorm_bwd_cl(const void *x, const void *dy, const float *w, void *dx, float *part, int64_t rows,
                            int c, float eps, int dtype, void *stream);
/* The same on the residual stream of a block (vmamba.py:384-396 under autograd): dx = LayerNorm-backward + gres (the gradient
 * that reaches the block input through the skip connection; NULL: none), and dxm (NULL: not wanted) = dx * mask[row /
 * rows_per_sample] -- the gradient of the PREVIOUS residual branch under stochastic depth (mask (B) f32 = keep / keep_prob
 * per sample; NULL: 1).  One pass where autograd issued the LayerNorm backward, an add and a multiply. */
int tramba_layernorm_bwd_res_cl(const void *x, const void *dy, const float *w, void *dx, float *part, const void *gres,
                                const float *mask, int64_t rows_per_sample, void *dxm, int64_t rows, int c, float eps,
                                int dtype, void *stream);
/* The general form behind the two entries above and tramba_shuffle_norm_bwd_cl (P > 1: dy is indexed through the pixel
 * shuffle of x's row). */
int tramba_layernorm_bwd_any_cl(const void *x, const void *dy, const float *w, void *dx, float *part, const void *gres,
                                const float *mask, int64_t rows_per_sample, void *dxm, int64_t rows, int c, float eps, int P,
                                int H, int W, int dtype, void *stream);
/* Training: backward of tramba_shuffle_norm_cl.  x (B, H, W, P*P*C) the un-shuffled input, dy (B, H*P, W*P, C) the gradient of
 * the shuffled, normalised map -> dx like x; part as tramba_layernorm_bwd_cl with rows = B*H*W*P*P.  The gradient is read
 * through the shuffle: no permuted copy of either map exists (modules.py:209-218, 687-696 under autograd). */
int tramba_shuffle_norm_bwd_cl(const void *x, const void *dy, const float *w, void *dx, float *part, int batch, int h,
                               int wd, int c, int p, float eps, int dtype, void *stream);
/* Residual add + stochastic depth + LayerNorm of the training path in one pass: xsum = x + y * mask[row / rows_per_sample]
 * (y NULL: no add, xsum unused), n = LayerNorm_C(xsum), n_act (NULL: not wanted) = act(n) -- the pre-activation / activation
 * pair a following `Linear(act(.))` needs under autograd.  x, y, xsum, n, n_act: (rows, C) dtype; w, b, mask f32. */
int tramba_add_layernorm_cl(const void *x, const void *y, const float *mask, int64_t rows_per_sample, const float *w,
                            const float *b, void *xsum, void *n, void *n_act, int64_t rows, int c, float eps, int act,
                            int dtype, void *stream);
/* The same launch with SS2D's z gate in the second store (training forward of the gated block): n_act = act(n) * silu(zpre),
 * zpre (rows, C) dtype = the gate's pre-activation; n_act is required.  xsum, the statistics and n are those of
 * tramba_add_layernorm_cl bit for bit. */
int tramba_add_layernorm_gate_cl(const void *x, const void *y, const float *mask, int64_t rows_per_sample, const float *w,
                                 const float *b, const void *zpre, void *xsum, void *n, void *n_act, int64_t rows, int c,
                                 float eps, int act, int dtype, void *stream);
/* Backward of p = gelu(n) * silu(zpre) from the two stored pre-activations: gn = gp * silu(zpre) * gelu'(n),
 * gz = gp * gelu(n) * silu'(zpre).  Pointwise over `count` < 2^31 elements of dtype, every tensor 16-byte aligned; three reads
 * and two writes per element, no atomics.  gn or gz may be gp itself (in place); n and zpre may not be written. */
int tramba_gelu_gate_bwd_cl(const void *gp, const void *n, const void *zpre, void *gn, void *gz, int64_t count, int dtype,
                            void *stream);
/* x: (B, H, W, P*P*C) -> y: (B, H*P, W*P, C) with y[b,hP+p1,wP+p2,:] = LN(x[b,h,w,(p1*P+p2)*C : +C]). */
int tramba_shuffle_norm_cl(const void *x, const float *w, const float *b, void *y, int batch, int h,
                           int wd, int c, int p, float eps, int dtype, void *stream);
/* shuffle_norm followed by a 1x1 convolution to ONE channel (FinalPatchExpand_X4 + the full-resolution
 * seg_layers head, Trambav6.py:132-137): y (B, H*P, W*P) f32 = <LayerNorm(shuffled row) rounded to dtype, head_w>
 * + head_b.  The normalised (B, H*P, W*P, C) map is never written. */
int tramba_shuffle_norm_head_cl(const void *x, const float *w, const float *b, const float *head_w, float head_b,
                                float *y, int batch, int h, int wd, int c, int p, float eps, int dtype,
                                void *stream);
/* Training: backward of tramba_shuffle_norm_head_cl in one pass over x (the normalised (B, H*P, W*P, C) map and its gradient
 * never exist).  g (B, H*P, W*P) f32 = d loss / d logits; dx (B, H, W, P*P*C) dtype; part (P, C + 4) f32 receives
 * P = tramba_shuffle_norm_head_bwd_parts() partial rows of A_c = sum over rows of g * xhat_c (slots 0..C) and G = sum g
 * (slot C); summed over the rows (tramba_slab_sum) they give d ln_w = head_w A, d ln_b = head_w G,
 * d head_w = ln_w A + ln_b G, d head_b = G.  C % 8 == 0 (4 for f32), C <= 512 (256). */
int64_t tramba_shuffle_norm_head_bwd_parts(int batch, int h, int wd, int c, int p, int dtype);
int tramba_shuffle_norm_head_bwd_cl(const void *x, const float *g, const float *ln_w, const float *head_w, void *dx,
                                    float *part, int batch, int h, int wd, int c, int p, float eps, int dtype, void *stream);
/* y[row] = <x[row, :], w> + bias: nn.Conv2d(C, 1, 1) on a channels-last map (decoder seg_layers,
 * Trambav6.py:62,67).  x (rows, C) dtype, w (C) f32, y (rows) f32. */
int tramba_rowdot_cl(const void *x, const float *w, float bias, float *y, int64_t rows, int c, int dtype,
                     void *stream);
/* Training: backward of tramba_rowdot_cl in one pass over x: gx (rows, C) dtype = gy[row] * w; part (P, C + 4) f32 receives P
 * partial rows, P = tramba_rowdot_bwd_parts(rows, c, dtype) (0: the shape is not served -- rows wider than 64 x 16 bytes),
 * columns 0 .. C = sum gy[row] * x[row, :] (the weight gradient), column C = sum gy[row] (the bias gradient); the caller sums
 * over P (tramba_slab_sum).  gy (rows) f32. */
int64_t tramba_rowdot_bwd_parts(int64_t rows, int c, int dtype);
int tramba_rowdot_bwd_cl(const void *x, const float *gy, const float *w, void *gx, float *part, int64_t rows, int c,
                         int dtype, void *stream);
/* Depth-wise stencils take TAP-MAJOR weights wt (ks*ks, C) f32 + bias bt (C) f32 produced by
 * tramba_dw_pack from the reference layout w (C, ks, ks), bias (C) or NULL.  With w3/b3/w5/b5
 * non-NULL (ks = 7) it packs the multi-scale stencil of DWMSMlp: identity + 3x3 + 5x5 + 7x7 folded
 * into one 7x7 (and b3 + b5 + b7), so y = GELU(h + dw3(h) + dw5(h) + dw7(h)) is ONE dwconv pass. */
int tramba_dw_pack(const float *w, const float *bias, const float *w3, const float *b3, const float *w5,
                   const float *b5, float *wt, float *bt, int c, int ks, void *stream);
/* `count` such packs in ceil(count / 40) launches (every depth-wise stencil of a model after an optimizer step): item i packs
 * w[i] (+ bias[i], and w3 / b3 / w5 / b5[i] for the folded multi-scale form; NULL entries as in tramba_dw_pack) into
 * wt[i] / bt[i].  All ten arguments are HOST arrays (device pointers, channel counts, kernel sizes); the items travel to the
 * kernel by value (hipGraph-capture safe). */
int tramba_dw_pack_multi(const float *const *w, const float *const *bias, const float *const *w3, const float *const *b3,
                         const float *const *w5, const float *const *b5, float *const *wt, float *const *bt, const int *c,
                         const int *ks, int count, void *stream);
/* Training path of the dense 3x3 convolutions of the VMamba stem / downsample layers (vmamba.py:454,481,486; the reference
 * gets their autograd from cuDNN through nn.Conv2d): the data movement around the library's GEMMs.
 *   im2col: x (B,H,W,C) dtype -> cols (B*Ho*Wo, CKp) dtype, column (ky*3 + kx)*C + ci (the k-major order of
 *           tramba_conv3x3s2_cl's weight), zeros in the padding taps and in columns 9C..CKp;  Ho = (H + 2 pad - 3)/stride + 1
 *   col2im: gcols (B*Ho*Wo, CKp) -> gx (B,H,W,C) = the adjoint gather (fp32 sums, fixed order, no atomics). */
int tramba_im2col3x3_cl(const void *x, void *cols, int batch, int h, int wd, int c, int stride, int pad, int ckp,
                        int dtype, void *stream);
int tramba_col2im3x3_cl(const void *gcols, void *gx, int batch, int h, int wd, int c, int stride, int pad, int ckp,
                        int dtype, void *stream);
/* Backward of F.interpolate(mode="bilinear", align_corners=False) from (planes, h, w) to (planes, hout, wout), fp32 -- the
 * resize of the deep-supervision outputs in the loss (train.py:76-85): gin = the adjoint, gathered per input pixel. */
int tramba_upsample_bilinear_bwd(const float *gout, float *gin, int planes, int h, int w, int hout, int wout,
                                 void *stream);
/* depth-wise ks x ks, stride 1, "same" padding, y = act(conv(x) + bt). */
int tramba_dwconv_cl(const void *x, const float *wt, const float *bt, void *y, int batch, int h,
                     int wd, int c, int ks, int act, int dtype, void *stream);
/* Training forms of the same stencil: y_pre (NULL: not wanted) also receives conv(x) + bt BEFORE the activation (the backward
 * of SiLU / GELU needs it; y = act of the value as stored); flip_taps = 1 mirrors the taps through the centre -- the input
 * gradient of the stencil is tramba_dwconv_dual_cl(gy, wt, zero bias, NULL, gx, ..., ACT_NONE, 1). */
int tramba_dwconv_dual_cl(const void *x, const float *wt, const float *bt, void *y_pre, void *y, int batch, int h, int wd,
                          int c, int ks, int act, int flip_taps, int dtype, void *stream);
/* The weight gradient of a stencil in the parameters' own layout: gwt (ks*ks + 1, C) f32 = tap-major taps + bias row (the
 * summed output of tramba_dwconv_wgrad_cl) -> g7 (C, ks*ks); with g5 / g3 non-NULL (ks = 7) the folded multi-scale stencil's
 * gradient restricted to the 5x5 / 3x3 parameters' supports (C, 25) / (C, 9) (the adjoint of tramba_dw_pack's fold); gb
 * (nb, C) or NULL = nb copies of the bias row. */
int tramba_dw_unpack_grad(const float *gwt, float *g7, float *g5, float *g3, float *gb, int nb, int c, int ks,
                          void *stream);
/* `count` such unpacks in ceil(count / 64) launches (the depth-wise parameter gradients of a whole backward pass: they are
 * leaves, nothing reads them before the optimizer); HOST arrays, items by value as in tramba_dw_pack_multi. */
int tramba_dw_unpack_grad_multi(const float *const *gwt, float *const *g7, float *const *g5, float *const *g3,
                                float *const *gb, const int *nb, const int *c, const int *ks, int count, void *stream);
/* Training: gradients of the same stencil w.r.t. its tap-major weights and bias (what autograd computes for
 * nn.Conv2d(groups=C), vmamba.py:301, 595-603).  part (P, ks*ks + 1, C) f32, P = tramba_dwconv_wgrad_parts(batch, h, wd,
 * c, ks): one partial row per workgroup (image, row band, column range), planes 0..ks*ks-1 = taps, last plane = bias; the
 * caller sums over P (tramba_slab_sum: fixed order).  The input gradient is tramba_dwconv_cl(gy, flipped taps, zero bias). */
int64_t tramba_dwconv_wgrad_parts(int batch, int h, int wd, int c, int ks);
int tramba_dwconv_wgrad_cl(const void *x, const void *gy, float *part, int batch, int h, int wd, int c, int ks,
                           int dtype, void *stream);
/* x: (B, n, n, C).  Y = Wy X Wx^T per channel; low = Y[:n/2,:n/2], high = Y[n/2:,n/2:],
 * both (B, n/2, n/2, C).  wx, wy: (n, n) f32.  tmp: (B, n, n, C) f32 workspace. */
int tramba_dct_split_cl(const void *x, const float *wx, const float *wy, float *tmp, void *high,
                        void *low, int batch, int n, int c, int dtype, void *stream);
/* y[m, :] = epilogue(x[m, :] @ W^T + bias);  x: (M, K) dtype, W: (N, K) dtype, bias (N) f32 or
 * NULL, y: (M, N) out_dtype.  act applied after bias.  residual (M, N) dtype or NULL is added
 * last.  MFMA path for f16/bf16. */
int tramba_linear_cl(const void *x, const void *w, const float *bias, const void *residual, void *y,
                     int64_t m, int n, int k, int act, int dtype, int out_dtype, void *stream);
/* LayerNorm2d followed by Linear2d as ONE launch (VSSBlock: norm -> op.in_proj, norm2 -> mlp.fc1, vmamba.py:384-396;
 * the decoder blocks likewise): y = epilogue(LayerNorm_K(x) @ W^T + b) computed as rstd_m * (x @ W'^T - mean_m * colsum) + t
 * with W' = W * gamma (rows of W scaled, in dtype), colsum (N) f32 = row sums of W' as rounded, bias (N) f32 = W beta + b.
 * The block derives mean / rstd of its own rows; the normalised map is never written.  16-bit dtypes, K % 64 == 0,
 * K <= 2048, N % 8 == 0; act / residual as tramba_linear_cl. */
int tramba_linear_ln_cl(const void *x, const void *w_folded, const float *colsum, const float *bias, const void *residual,
                        void *y, int64_t m, int n, int k, float eps, int act, int dtype, int out_dtype, void *stream);
/* Same with the K dimension of x split over two tensors, x = [x1 (M, k1) | x2 (M, k - k1)]: Linear2d applied to
 * torch.cat((x1, x2), dim=-1) without materialising the concatenation (decoder concat_back_dim, Trambav6.py:124;
 * FreqSS2Dv6, freq_mamba.py:52).  16-bit dtypes, k1 % 64 == 0 and (k - k1) % 64 == 0. */
int tramba_linear2_cl(const void *x1, const void *x2, int k1, const void *w, const float *bias, const void *residual,
                      void *y, int64_t m, int n, int k, int act, int dtype, int out_dtype, void *stream);
/* Row statistics handed from the GEMM that writes a map to the LayerNorm-folded GEMM that reads it next (16-bit inference:
 * fc2 + residual -> norm -> in_proj, out_proj + residual -> norm2 -> fc1).
 * Producer (tramba_linear_rowstat_cl / tramba_linear2_rowstat_cl = the plain / two-source GEMM with one more output):
 * rowstat_out, a float2 slab (M, ceil(N / 64)), receives per row and 64-column tile (sum, sum of squares) of the valid
 * columns of y as rounded to the output dtype -- fp32, fixed order, no atomics, rows below M only.  *emitted = 1 when the
 * slab was written; 0 when the form planned for the call cannot write it (weight-stationary form, fp32 output, K that is no
 * multiple of 64): the slab is then untouched and the caller goes on without statistics.  rowstat_out = NULL: the plain call.
 * Consumer (tramba_linear_ln_rowstat_cl): rowstat_in, such a slab over ITS input rows with p = K / 64 partials per row; the
 * block folds them in ascending order into mean = S1 / K, rstd = rsqrt(max(S2 / K - mean^2, 0) + eps) instead of deriving
 * them from its staged tiles in every column tile, and may then run the form the plain GEMM of the shape runs.  The weight-
 * stationary form keeps deriving its own.  rowstat_in = NULL: tramba_linear_ln_cl, bit for bit. */
int tramba_linear_rowstat_cl(const void *x, const void *w, const float *bias, const void *residual, void *y, int64_t m,
                             int n, int k, int act, int dtype, int out_dtype, float *rowstat_out, int *emitted, void *stream);
int tramba_linear2_rowstat_cl(const void *x1, const void *x2, int k1, const void *w, const float *bias, const void *residual,
                              void *y, int64_t m, int n, int k, int act, int dtype, int out_dtype, float *rowstat_out,
                              int *emitted, void *stream);
int tramba_linear_ln_rowstat_cl(const void *x, const void *w_folded, const float *colsum, const float *bias,
                                const void *residual, void *y, int64_t m, int n, int k, float eps, int act, int dtype,
                                int out_dtype, const float *rowstat_in, int p, void *stream);

/* y_pre = x @ w^T + bias and y_act = act(y_pre) from ONE launch (act = GELU or SiLU): the forward of `act(Linear(x))` on the
 * training path, whose backward needs the pre-activation (Models/modules.py:134-153 under autograd).  16-bit dtypes,
 * K % 64 == 0, N % 8 == 0; both outputs (M, N) in dtype. */
int tramba_linear_dual_cl(const void *x, const void *w, const float *bias, void *y_pre, void *y_act, int64_t m, int n,
                          int k, int act, int dtype, void *stream);
/* Weight (and bias) gradient of a 1x1 convolution under autograd -- what `loss.backward()` computes for every
 * Linear2d (Models/modules.py:10-19; the reference gets it from cuDNN/cuBLAS through F.conv2d's autograd):
 *   out[g][n*K + k]  = sum over batches b and tokens t of gy[g][b][t][n] * x[g][b][t][k]       (N x K, fp32)
 *   out[g][N*K + n]  = sum over b, t of gy[g][b][t][n]                                          (bias gradient, if want_bias)
 * Element (g, b, t, c) of an operand sits at base + b*bs + g*gs + t*ld + c (element strides): groups / nbatch serve the
 * per-direction contractions of the SS2D backward on (B, K, L, C) tensors; a plain Linear2d has groups = nbatch = 1.
 * out: (groups, N*K + N) f32.  workspace: tramba_wgrad_workspace() bytes of fp32 partial slabs (the token range is split
 * over workgroups, slabs are summed in a fixed order).  16-bit dtypes; N, K and every stride multiples of 8. */
size_t tramba_wgrad_workspace(int64_t m, int n, int k, int groups, int nbatch);
int tramba_wgrad_cl(const void *gy, const void *x, float *out, void *workspace, size_t workspace_bytes, int64_t m, int n,
                    int k, int groups, int nbatch, int64_t gy_bs, int64_t gy_gs, int gy_ld, int64_t x_bs, int64_t x_gs,
                    int x_ld, int want_bias, int dtype, void *stream);
/* The same launch stopped at the partial slabs: *nslab = slabs per group left in `workspace` as (groups, *nslab, N*K + N)
 * fp32, or 0 when a single slab was written straight to `out`.  The caller sums them later -- tramba_slab_sum, or
 * tramba_multi_sum together with the other pending sums of a training step (the gradient of a Linear2d hangs off the backward
 * chain: nothing reads it before the optimizer, reference train.py:86-89). */
int tramba_wgrad_parts_cl(const void *gy, const void *x, float *out, void *workspace, size_t workspace_bytes, int64_t m,
                          int n, int k, int groups, int nbatch, int64_t gy_bs, int64_t gy_gs, int gy_ld, int64_t x_bs,
                          int64_t x_gs, int x_ld, int want_bias, int dtype, void *stream, int *nslab);
/* y[z][t][0..N) = x[z][t][:] . w[z % groups][n][:]  for z < nz, t < m: x (nz, m, K) dtype, w (groups, N, K) dtype,
 * y fp32 rows of stride ldy (>= N; the columns past N are left untouched).  N <= 64, K % 8 == 0.  The dt_rank projection
 * of the SS2D backward (vmamba.py:236 under autograd): d(x_dbl ranks) = d(dt_raw) @ dt_projs_weight[k]. */
int tramba_rows_gemm_cl(const void *x, const void *w, float *y, int nz, int64_t m, int n, int k, int groups, int ldy,
                        int dtype, void *stream);
/* The 16-bit copies of a model's fp32 master weights that the next training step reads (the reference keeps fp32 weights
 * and lets autocast cast per call, Trambav6.py:151-154 / train.py:74-89): for every table entry t,
 *   dst[t] (rows, cols) = (dtype) src[t],   dst_t[t] (cols, rows) = its transpose      (either pointer may be 0: skipped)
 * table: DEVICE array of ntensors x 8 int64 {src, dst, dst_t, rows, cols, first_tile, dst_ld, dst_t_ld}; src is a dense
 * (rows, cols) matrix, the rows of dst / dst_t are dst_ld / dst_t_ld elements apart (= cols / rows for dense outputs;
 * larger when the matrix is a block of a padded layout, e.g. one direction of the x_proj weight); a tensor owns
 * ceil(rows/64)*ceil(cols/64) consecutive tiles starting at first_tile (ascending), total_tiles = their sum.  8-byte
 * alignment of every dst / dst_t row start when the leading dimensions are multiples of 4. */
int tramba_shadow_cast_multi(const void *table, int ntensors, int64_t total_tiles, int dtype, void *stream);
/* out[i] = sum over s < nslab of part[s*n + i], i < n, summed in slab order (deterministic): the per-workgroup partial sums
 * of the LayerNorm / depth-wise / scan parameter gradients.  n % 4 == 0, 16-byte aligned. */
int tramba_slab_sum(const float *part, float *out, int64_t n, int nslab, void *stream);
/* `count` such sums in ceil(count / 64) launches: outs[i][j] = sum over s < nslab[i] of parts[i][s*n[i] + j], the same
 * summation order as tramba_slab_sum / the slab sums of tramba_wgrad_cl.  parts / outs / n / nslab are HOST arrays of device
 * pointers and sizes (they travel to the kernel by value: nothing is copied to the device, hipGraph-capture safe).
 * _strided: slab s of table i starts stride[i] floats after slab s - 1 (>= n[i], a multiple of 4; NULL = dense) -- a row range
 * of a wider table summed straight into its place in another layout (the x_proj weight gradient leaves the GEMM in the scan
 * kernels' padded layout and lands in the parameter's own, vmamba.py:236: no concatenation kernel). */
int tramba_multi_sum_strided(const float *const *parts, float *const *outs, const int64_t *n, const int64_t *stride,
                             const int *nslab, int count, void *stream);
int tramba_multi_sum(const float *const *parts, float *const *outs, const int64_t *n, const int *nslab, int count,
                     void *stream);

/* The whole last decoder stage in one kernel (FinalPatchExpand_X4 + seg_layers[-1], Trambav6.py:132-137):
 * y (B, H*P, W*P) f32 = head(LayerNorm_128(pixel_shuffle_P(x @ w^T))).  x (B, H, W, Cin) dtype, w (P*P*128, Cin) dtype
 * (the expand Linear2d, no bias), ln_w / ln_b / head_w (128) f32.  16-bit dtypes, Cin % 64 == 0. */
int tramba_expand_norm_head_cl(const void *x, const void *w, const float *ln_w, const float *ln_b,
                               const float *head_w, float head_b, float *y, int batch, int h, int wd, int cin, int p,
                               float eps, int dtype, void *stream);

/* ------------------------------------------------------------------ dense convs of the VMamba stem */
/* Implicit-GEMM 3x3 / stride 2 / pad 1 convolution on a channels-last map (patch_embed[5] and the three
 * downsample convs, Models/vmamba.py:454,486): x (B, Hin, Win, Cin) -> y (B, ceil(Hin/2), ceil(Win/2), Cout).
 * w is K-major (Cout, 3, 3, Cin) = reference weight.permute(0,2,3,1), same dtype as x; Cin % 64 == 0. */
int tramba_conv3x3s2_cl(const void *x, const void *w, const float *bias, void *y, int batch, int hin,
                        int win, int cin, int cout, int dtype, void *stream);
/* patch_embed[0..4] fused (vmamba.py:481-485): conv 3x3/s2/p1 (3 -> 64) + bias + LayerNorm2d(64) + GELU.
 * img (B, 3, H, W) NCHW in f32 or `dtype`; w (64, 3, 3, 3) f32 reference layout; y (B, H/2, W/2, 64). */
int tramba_stem_conv_ln_gelu(const void *img, const float *w, const float *bias, const float *ln_w,
                             const float *ln_b, void *y, int batch, int h, int wd, float eps,
                             int img_dtype, int dtype, void *stream);

/* ------------------------------------------------------------------ evaluation (train.py:101-139 test_one_epoch) */
/* Per-image statistics of saliency maps against their masks, from which MAE, F-measure, E-measure and S-measure of
 * Evaluation/metrics.py follow without the maps leaving the GPU.  pred (B, H, W) f32 = sigmoid(logits) (NOT yet
 * min-max normalised: the kernel does Evaluation/metrics.py:13-19 itself); gt (B, H, W) u8, 0 / 1.
 * ints (B, TRAMBA_EVAL_NINT) i64: [0] mask area, [1] sum g*col, [2] sum g*row, [3] cx, [4] cy (S-measure centroid, 1-based
 *   split point as metrics.py:201-212), [5] / [6] pixels >= adaptive threshold inside / outside the mask, [7] H*W,
 *   [8 .. 264) histogram of uint8(p*255) inside the mask, [264 .. 520) outside.
 * dbl (B, TRAMBA_EVAL_NDBL) f64: [0] min, [1] max of pred, [2] sum p, [3] sum |p - g|, [4] [5] sum p, p^2 inside the mask,
 *   [6] [7] sum (1-p), (1-p)^2 outside, [8 + 4q + {0,1,2,3}] sum p, p^2, g, p*g over quadrant q (LT, RT, LB, RB),
 *   [24] the adaptive threshold, [32 + 3q + {0,1,2}] centred sums over quadrant q: (p - mean p)^2, (g - mean g)^2,
 *   (p - mean p)(g - mean g), [44] sum (p - mean)^2 inside the mask, [45] sum ((1-p) - mean)^2 outside;
 *   p = normalised prediction.  NaN where a region is empty, as numpy gives. */
#define TRAMBA_EVAL_NINT 520
#define TRAMBA_EVAL_NDBL 48
int tramba_saliency_stats(const float *pred, const unsigned char *gt, long long *ints, double *dbl, int batch, int h,
                          int w, void *stream);
/* The weighted F-measure (Evaluation/metrics.py:379-441), in two steps.  1 <= h, w <= TRAMBA_WFM_MAX_DIM, batch <= 65535.
 * Exact Euclidean feature transform of gt (B, H, W) u8 (0 / non-zero), the one metrics.py:391 takes from
 * scipy.ndimage.distance_transform_edt(gt == 0, return_indices=True): idx (B, H, W) i32 = r * W + c of the nearest mask
 * pixel (identical to scipy's indices, ties included: Maurer's separable algorithm as scipy runs it), dist2 (B, H, W) i32 =
 * its squared distance.  An image with an empty mask gets idx = dist2 = -1 everywhere. */
#define TRAMBA_WFM_MAX_DIM 4096
int tramba_feature_transform(const unsigned char *gt, int *idx, int *dist2, int batch, int h, int w, void *stream);
/* sums (B, 3) f64 per image = { sum gt, sum Ew[gt], sum Ew[~gt] } of metrics.py:393-419 (then R = 1 - sums[1] / sums[0],
 * P = TPw / (TPw + sums[2] + eps) with TPw = sums[0] - sums[1], on the host): pred (B, H, W) f32 min-max normalised in fp32
 * (metrics.py:13-19), E = |p - g|, Et = E of the nearest mask pixel (idx / dist2 from the feature transform of the same gt),
 * EA = 7x7 filter of Et with zero padding (fp64 accumulation, fp32 result), MIN_E_EA, B = 2 - exp(ln(0.5) / 5 * dist) in
 * fp64, Ew = MIN_E_EA * B.  gauss: HOST array of the 49 filter weights, row-major (matlab_style_gauss2D, metrics.py:429-441);
 * it travels by value.  workspace: device memory of the size the workspace query returns.  Fixed summation order: bitwise
 * reproducible, independent of the batch an image is in.  An empty mask gives sums = 0. */
size_t tramba_weighted_f_workspace(int batch, int h, int w);
int tramba_weighted_f_sums(const float *pred, const unsigned char *gt, const int *idx, const int *dist2, const double *gauss,
                           double *sums, void *workspace, size_t workspace_bytes, int batch, int h, int w, void *stream);

/* ------------------------------------------------------------------ deployment: frames in, saliency maps out */
/* Camera frames to model input, bit for bit the loader's test transform (data/dataloader.py:22-39 get_transform(S, 'Test'):
 * custom_transforms.py Resize(BILINEAR) + ToTensor/Normalize).  The resize is PIL's separable 8-bit bilinear resample
 * (horizontal pass into a u8 intermediate, then vertical; fixed-point weights with 22 fractional bits; an axis whose size
 * does not change is copied), the normalisation f = u8 / 255 in fp32, t = fp32(f - mean[c]), out = fp32(t / std[c]) with
 * mean / std in fp64.  Sizes: 1 <= in_h, in_w <= TRAMBA_FRAME_MAX_DIM, 1 <= out_h, out_w <= TRAMBA_FRAME_MAX_OUT.
 * tramba_resize_table fills the HOST int32 table for one (frame size, output size) pair, in fp64 on the host:
 * tramba_resize_table_words() words (0: sizes rejected); the caller uploads it once and reuses it.
 * tramba_frames_to_input: frames (B, in_h, in_w, 3) u8 contiguous, RGB (bgr = 0) or BGR (bgr = 1); table: the DEVICE copy of
 * the table for these sizes; out (B, 3, out_h, out_w) f32, channels in RGB order.  batch <= 65535. */
#define TRAMBA_FRAME_MAX_DIM 16384
#define TRAMBA_FRAME_MAX_OUT 2048
size_t tramba_resize_table_words(int in_h, int in_w, int out_h, int out_w);
int tramba_resize_table(int in_h, int in_w, int out_h, int out_w, const double *mean, const double *std, int *table,
                        size_t words);
int tramba_frames_to_input(const unsigned char *frames, const int *table, float *out, int batch, int h, int w, int out_h,
                           int out_w, int bgr, void *stream);
/* Logits to saliency maps at the frame's size (test_TSOD.py:61-66): logits (B, 1, in_h, in_w) f32 / f16 / bf16 (dtype), out
 * (B, h, w) u8 = uint8(sigmoid(F.interpolate(logits.float(), (h, w), mode='bilinear', align_corners=False)) * 255), with
 * torch's source-index and lambda arithmetic.  1 <= in_h, in_w <= TRAMBA_FRAME_MAX_OUT, 1 <= h, w <= TRAMBA_FRAME_MAX_DIM,
 * batch <= 65535. */
int tramba_logits_to_u8(const void *logits, unsigned char *out, int batch, int in_h, int in_w, int h, int w, int dtype,
                        void *stream);
/* The same two ends for a batch of frames of DIFFERENT sizes (a dataset folder).  packed (device, packed_bytes, 16-byte
 * aligned): batch descriptors of TRAMBA_FRAMES_DESC_WORDS int64 words, then the tramba_resize_table words of every frame
 * size to (size, size) and the u8 frames (h, w, 3) at the byte offsets the descriptors name.  Words of a descriptor: frame
 * offset, h, w, table offset (a multiple of 4), taps per output column, taps per output row, offset of the frame's (h, w) map
 * in the output buffer (a multiple of 16, increasing, maps disjoint), then (float)size / (float)h and (float)size / (float)w
 * as fp32 bits; the rest 0.  Frame i's input plane and map are bit for bit what the uniform entries give for that frame alone.
 * Launch geometry and kernel arguments depend on (batch, size, out_capacity) only, never on the frame sizes, so one captured
 * graph serves every packed batch that fits its buffers.  desc_host: a HOST copy of the descriptors, checked before the launch.
 * tramba_frames_ragged_check is that check alone (no launch), for a caller that replays a graph: sides 1 ..
 * TRAMBA_FRAME_MAX_DIM, 3 <= size <= TRAMBA_FRAME_MAX_OUT, batch <= 65535; parts & TRAMBA_RAGGED_IN: frames and tables inside
 * packed_bytes and outside the descriptor area, taps those of the sizes; parts & TRAMBA_RAGGED_OUT: map offsets aligned,
 * increasing, not overlapping, every map inside out_capacity, scale words those of the sizes.
 * tramba_frames_to_input_ragged: out (batch, 3, size, size) f32.  tramba_logits_to_u8_ragged: logits (batch, 1, size, size)
 * f32 / f16 / bf16, out a u8 buffer of out_capacity bytes (16-byte aligned) that receives the maps at their offsets; bytes
 * between maps and after the last one are not written.  No allocation, copy or synchronisation in either. */
#define TRAMBA_FRAMES_DESC_WORDS 16
#define TRAMBA_RAGGED_IN 1
#define TRAMBA_RAGGED_OUT 2
int tramba_frames_ragged_check(const int64_t *desc_host, int batch, int size, size_t packed_bytes, size_t out_capacity,
                               int parts);
int tramba_frames_to_input_ragged(const unsigned char *packed, const int64_t *desc_host, size_t packed_bytes, float *out,
                                  int batch, int size, int bgr, void *stream);
int tramba_logits_to_u8_ragged(const void *logits, const unsigned char *packed, const int64_t *desc_host, unsigned char *out,
                               size_t out_capacity, int batch, int size, int dtype, void *stream);

/* ------------------------------------------------------------------ training: uint8 pairs in, train batches out */
/* The train transform of the loader (data.get_transform(S, 'train'): static resize, scale-crop, mirror, rotation, the three
 * enhancers, to_tensors) on the device, bit for bit, for draws made on the host (tramba_amd/augment.py).  Tables (HOST int32
 * arrays, fp64 with contraction off; the caller uploads them once and caches them):
 *   tramba_augment_source_table: one source size (h, w) -> (size, size): {kx, ky, 0, 0}, the tramba_resize_table words of
 *     the bilinear image resize, then Pillow's nearest indices of the mask, x[size] then y[size] (-1: fill 0);
 *   tramba_augment_size_table: one output side: the normalisation table [3][256] f32, u / 255 [256] f32, SMOOTH / 13 [9] f32
 *     (words 1024..), {lo, hi} at word 1040, then at 1042 the word offset of the bicubic axis table (bounds[R][2],
 *     weights[R][taps]) of every R in lo .. hi (0 for R == size, Pillow's copy); taps: tramba_augment_scale_taps;
 *   tramba_augment_rotation: Image.rotate(degrees, expand=True) + centre crop as 6 16.16 words A0..A5 (source pixel of
 *     output (x, y) = ((A0 x + A1 y + A2) >> 16, (A3 x + A4 y + A5) >> 16); out of range: 0).
 * tramba_augment_batch: packed (device, packed_bytes): batch descriptors of TRAMBA_AUG_DESC_WORDS int64 words (layout:
 * csrc/augment.hip), then the u8 images (h, w, 3) and masks (h, w) at the byte offsets they name; desc_host: a host copy of
 * the descriptors, checked before any launch (sizes 1 .. TRAMBA_FRAME_MAX_DIM, 3 <= size <= TRAMBA_FRAME_MAX_OUT, offsets
 * inside the buffer, draws in range).  image (batch, 3, size, size) f32, label (batch, 1, size, size) f32.  Four launches on
 * `stream`, no allocation, no synchronisation; each sample's result is independent of the batch it is in. */
#define TRAMBA_AUG_DESC_WORDS 32
#define TRAMBA_AUG_CONTRAST 0
#define TRAMBA_AUG_BRIGHTNESS 1
#define TRAMBA_AUG_SHARPNESS 2
size_t tramba_augment_source_table_words(int h, int w, int size);
int tramba_augment_source_table(int h, int w, int size, int *table, size_t words);
size_t tramba_augment_size_table_words(int size);
int tramba_augment_size_table(int size, const double *mean, const double *std, int *table, size_t words);
int tramba_augment_scale_taps(int size, int r);
int tramba_augment_rotation(int size, int degrees, int *coef);
size_t tramba_augment_workspace(int batch, int size);
int tramba_augment_batch(const unsigned char *packed, const int64_t *desc_host, size_t packed_bytes, const int *size_table,
                         float *image, float *label, void *workspace, size_t workspace_bytes, int batch, int size,
                         void *stream);

/* ------------------------------------------------------------------ loss and optimizer of the training step */
/* The deep-supervision loss (train.py:76-85; utils/loss.py:6-11) of ONE output: logits (planes, h, w) f32 bilinearly resized
 * (F.interpolate(mode="bilinear"), align_corners=False; identity when the sizes agree) to the label (planes, hout, wout) f32,
 * then per plane the three sums behind binary_cross_entropy_with_logits + iou_loss:
 *   part[plane][blk][0..3) = sum of { max(z,0) - z y + log(1 + exp(-|z|)),  sigmoid(z) y,  sigmoid(z) + y }
 * over the pixels workgroup blk of nblk walked (any nblk >= 1; fixed summation order).  The resized map is never stored. */
int tramba_sod_loss_sums(const float *logits, const float *label, float *part, int planes, int h, int w, int hout, int wout,
                         int nblk, void *stream);
/* loss[0] = sum over outputs o < nout (<= 8) of weights[o] * ( mean bce + mean over planes of 1 - (I + 1) / (U - I + 1) ),
 * from the tables of tramba_sod_loss_sums (parts[o]: (planes, nblk[o], 3)), accumulated in fp64, and coefs[o] (planes, 4) f32 =
 * the per-plane coefficients { a, cI, cU, 0 } of d loss / d resized logit = a (p - y) + p (1 - p) (cI y + cU).
 * parts / nblk / weights (NULL: all 1) / coefs are HOST arrays; they travel by value (hipGraph-capture safe).
 * planes <= 512; npix = hout * wout. */
int tramba_sod_loss_finish(const float *const *parts, const int *nblk, const float *weights, float *const *coefs, int nout,
                           int planes, int64_t npix, float *loss, void *stream);
/* glogits (planes, h, w) f32 = gscale[0] * d loss / d logits of one output (gscale: device scalar, the incoming gradient of
 * the loss; NULL = 1).  A resized output goes through the adjoint of the bilinear resize, which is separable: the gradient
 * at label resolution is formed once per label pixel in LDS, folded along x into `workspace` (planes, hout, w) f32 and then
 * along y (no atomics, fixed order; cf. tramba_upsample_bilinear_bwd).  hout >= h, wout >= w, wout <= 4096. */
size_t tramba_sod_loss_grad_workspace(int planes, int h, int w, int hout, int wout);
int tramba_sod_loss_grad(const float *logits, const float *label, const float *coef, const float *gscale, float *glogits,
                         void *workspace, size_t workspace_bytes, int planes, int h, int w, int hout, int wout, void *stream);
/* ---- the weighted losses: structure_loss (utils/loss.py:14-34) and wbce (utils/loss.py:37-42) ----
 * weit (planes, h, w) f32 = 1 + 5 |avg_pool2d(label, k, stride 1, padding k / 2) - label| (utils/loss.py:22 with k = 31,
 * utils/loss.py:39 with k = 15): zero padding, divisor k * k everywhere (count_include_pad, torch's default).  Odd k <= 63, any
 * h, w >= 1 (windows larger than the image included), labels any floats.  Separable sums in LDS, fixed order, plain stores. */
int tramba_loss_weight_map(const float *label, float *weit, int planes, int h, int w, int k, void *stream);
/* The weighted forms of the three entries above, through the same kernels: arguments, limits, workspace, host arrays by
 * value and summation order as there.  wmap (planes, hout, wout) f32 is the map of tramba_loss_weight_map (W = wmap) or, with
 * weight_is_raw != 0, the caller's `weight` of utils/loss.py:23-24 (W = 1 + 5 wmap); the BCE target is smoothed,
 * yhat = (1 - eps) y + eps / 2 with 0 <= eps < 1 (utils/loss.py:16-19, 26; eps = 0.001 for structure_loss, 0 for wbce).
 * Sums:   part[plane][blk][0..5) = sum of { bce(z, yhat),  W bce(z, yhat),  W,  W sigmoid(z) y,  W (sigmoid(z) + y) }
 *         (utils/loss.py:27-28, 30-32; y unsmoothed in the last two, as there). */
int tramba_sod_wloss_sums(const float *logits, const float *label, const float *wmap, float *part, int planes, int h, int w,
                          int hout, int wout, int nblk, float eps, int weight_is_raw, void *stream);
/* Finish: parts[o]: (planes, nblk[o], 5).  With I = sum W p y, U = sum W (p + y):
 *   loss[0] = sum_o weights[o] * ( BCE term + [with_iou] mean over planes of 1 - (I + 1) / (U - I + 1) )       (utils/loss.py:33-34)
 *   per_pixel == 0: BCE term = sum bce / (planes npix) -- utils/loss.py:27 AS IT EXECUTES: `reduce='none'` is the legacy
 *                   argument and a non-empty string is true, so the call returns the batch mean and W cancels in line 28;
 *   per_pixel != 0: BCE term = mean over planes of (sum W bce) / (sum W) -- lines 27-28 with reduction='none', as published.
 * coefs[o] (planes, 4) f32 = { a, cI, cU, per_pixel } of d loss / d resized logit = a omega (p - yhat) + p (1 - p) W (cI y + cU),
 * omega = W when per_pixel, else 1;  with_iou == 0 (wbce): cI = cU = 0. */
int tramba_sod_wloss_finish(const float *const *parts, const int *nblk, const float *weights, float *const *coefs, int nout,
                            int planes, int64_t npix, int per_pixel, int with_iou, float *loss, void *stream);
/* Gradient (autograd through utils/loss.py:26-34): reads the weight map as well; eps / weight_is_raw as given to the sums. */
size_t tramba_sod_wloss_grad_workspace(int planes, int h, int w, int hout, int wout);
int tramba_sod_wloss_grad(const float *logits, const float *label, const float *wmap, const float *coef, const float *gscale,
                          float *glogits, void *workspace, size_t workspace_bytes, int planes, int h, int w, int hout, int wout,
                          float eps, int weight_is_raw, void *stream);
/* One Adam step (torch.optim.Adam as train.py:266-280 builds it: amsgrad off, maximize off) on `count` fp32 tensors:
 *   steps[i][0] += 1 (device counters, part of the optimizer's state_dict);  g += weight_decay p;
 *   exp_avg = lerp(exp_avg, g, 1 - beta1);  exp_avg_sq = beta2 exp_avg_sq + (1 - beta2) g g;
 *   p -= lr / (1 - beta1^t) * exp_avg / (sqrt(exp_avg_sq) / sqrt(1 - beta2^t) + eps)       (bias corrections in fp64)
 * The six arrays are HOST arrays of device pointers / element counts; the tensors travel to the kernels by value, 72 per
 * launch (nothing is copied to the device: hipGraph-capture safe).  Any alignment; 16-byte aligned tensors take the
 * vector path. */
int tramba_adam_step(float *const *params, const float *const *grads, float *const *exp_avg, float *const *exp_avg_sq,
                     float *const *steps, const int64_t *numel, int count, double lr, double beta1, double beta2, double eps,
                     double weight_decay, void *stream);
/* ---- step control: gradient accumulation, norm clipping and the skip of a non-finite step, decided on the device ----
 * (No reference counterpart: train.py steps once per batch.)  The record lives in device memory, owned by the caller; the
 * entries below read and write it, so that a replayed hipGraph of a whole optimisation step needs no host value that changes
 * from step to step.  Zero-filled = "no micro-batch yet, nothing skipped". */
typedef struct tramba_step_ctl {
    float norm;              /* L2 norm of the MEAN gradient before clipping (what torch's clip_grad_norm_ returns) */
    float scale;             /* what the optimizer multiplies the accumulated gradient by: mean_scale * clip factor */
    int32_t skip;            /* 1: an element was Inf / NaN and the caller asked for skipping -- the optimizer changes nothing */
    int32_t micro;           /* micro-batches accumulated since the last tramba_grad_norm */
    int64_t skipped_steps;   /* steps skipped since the record was zeroed */
} tramba_step_ctl;
/* acc[i] = grads[i] when ctl->micro == 0, else acc[i] += grads[i] (fp32, element-wise: the accumulated value is the
 * micro-batch gradients added in micro-batch order); then ctl->micro += 1 (a one-lane launch behind the others).
 * grads[i] == NULL: the micro-batch produced no gradient for tensor i -- zeros (stored on the first micro-batch, nothing
 * to add later).  HOST arrays, tensors by value (128 per launch), any alignment, 16-byte aligned pairs take the vector path. */
int tramba_grad_accumulate(float *const *acc, const float *const *grads, const int64_t *numel, int count,
                           tramba_step_ctl *ctl, void *stream);
/* The global L2 norm over `count` fp32 tensors and the decisions that hang on it, written into the record:
 *   norm  = sqrt(sum of squares) * mean_scale         squares formed and added in fp64, per chunk of 8192 elements, the
 *                                                     partials added by one block in a fixed order (no atomics)
 *   skip  = skip_nonfinite && any element Inf / NaN   (decided per element, not from the norm)
 *   scale = mean_scale * min(1, max_norm / (norm + 1e-6))     (torch.nn.utils.clip_grad_norm_;  max_norm <= 0: mean_scale)
 *   skipped_steps += skip;  micro = 0.
 * mean_scale > 0 is 1 / micro-batches.  workspace: tramba_grad_norm_workspace() bytes, 8-byte aligned. */
size_t tramba_grad_norm_workspace(const int64_t *numel, int count);
int tramba_grad_norm(const float *const *grads, const int64_t *numel, int count, double mean_scale, double max_norm,
                     int skip_nonfinite, tramba_step_ctl *ctl, void *workspace, size_t workspace_bytes, void *stream);
/* tramba_adam_step with two device scalars (either may be NULL; both NULL is tramba_adam_step bit for bit):
 *   gscale: g = gscale[0] * g in fp32 before the weight decay and everything else;
 *   skip:   skip[0] != 0 -- the call changes nothing: parameters, both moments and the step counters keep their bits.
 * Both are read by the kernels when they run (a replayed graph follows the record, not the values at capture). */
int tramba_adam_step_ctl(float *const *params, const float *const *grads, float *const *exp_avg, float *const *exp_avg_sq,
                         float *const *steps, const int64_t *numel, int count, double lr, double beta1, double beta2,
                         double eps, double weight_decay, const float *gscale, const int *skip, void *stream);
/* ---- dynamic loss scaling (fp16 training): the scale lives on the device and moves after every optimizer step ----
 * A second record, owned by the caller like tramba_step_ctl.  `scale` is what the gradient of the loss is multiplied by
 * (the caller hands &scale to the loss gradient kernels as their `gscale`); it is always a power of two, so `inv_scale`
 * is exact and un-scaling changes no bit of a gradient that neither over- nor underflowed.  The caller fills scale and
 * inv_scale before the first step (zeros are not a valid state). */
typedef struct tramba_loss_scale {
    float scale;             /* 2^k: the loss gradient is multiplied by it */
    float inv_scale;         /* 1 / scale, exact */
    int32_t good_steps;      /* optimizer steps since the scale last changed that were not skipped */
    int32_t reserved;
    int64_t backoffs;        /* times the scale was cut since the record was filled */
} tramba_loss_scale;
/* tramba_grad_norm on gradients that carry ls->scale: the same two kernels, the same fp64 partial sums and per-element
 * Inf / NaN flags; the finishing block reads ls->inv_scale on the device and writes
 *   norm  = sqrt(sum of squares) * mean_scale * inv_scale                     (the norm of the UNSCALED mean gradient)
 *   scale = mean_scale * inv_scale * min(1, max_norm / (norm + 1e-6))         (what tramba_adam_step_ctl multiplies in)
 * ls == NULL is tramba_grad_norm bit for bit. */
int tramba_grad_norm_scaled(const float *const *grads, const int64_t *numel, int count, double mean_scale, double max_norm,
                            int skip_nonfinite, tramba_step_ctl *ctl, const tramba_loss_scale *ls, void *workspace,
                            size_t workspace_bytes, void *stream);
/* The scale's move after a step (a one-lane launch behind the optimizer's; reads ctl->skip on the device):
 *   skipped:  scale = max(min_scale, scale * backoff), good_steps = 0, backoffs += 1;
 *   else:     good_steps += 1; at growth_interval: scale = min(max_scale, scale * growth), good_steps = 0;
 *   inv_scale = 1 / scale.
 * growth > 1, backoff < 1, min_scale <= max_scale: powers of two that fp32 holds as normal numbers together with their
 * inverses (2^-126 .. 2^126); growth_interval >= 1.  Anything else is refused (< 0, tramba_last_error()). */
int tramba_loss_scale_update(tramba_loss_scale *ls, const tramba_step_ctl *ctl, double growth, double backoff,
                             int growth_interval, double min_scale, double max_scale, void *stream);
/* ---- per-step learning-rate schedule and weight average: a third record, owned by the caller like the other two ----
 * (No reference counterpart: utils/lr.py changes the rate at listed epochs, on the host.)  The optimizer kernel reads the
 * record when it runs, so a replayed hipGraph follows a schedule that moves at every step.  The caller fills the record
 * before the first step (step, the factor and the weight of that step). */
typedef struct tramba_step_sched {
    int64_t step;            /* optimizer steps ATTEMPTED since the record was filled (skipped ones included) */
    double lr_factor;        /* what every group's lr is multiplied by in the step under way */
    float ema_weight;        /* w of  ema += w * (p - ema)  in the step under way */
    int32_t reserved;
} tramba_step_sched;
/* The record's move after a step (a one-lane launch behind the optimizer's and behind tramba_loss_scale_update):
 *   step += 1;  lr_factor = lr_table[min(step, n_lr - 1)];  ema_weight = ema_table[min(step, n_ema - 1)].
 * lr_table: doubles, ema_table: floats, both in device memory.  lr_table == NULL: lr_factor = 1.0; ema_table == NULL:
 * ema_weight stays.  The move does not look at the skip flag: a schedule ends at the step it was planned to end at.
 * A non-NULL table with n < 1 is refused (< 0, tramba_last_error()).  No allocation, no synchronisation. */
int tramba_step_sched_advance(tramba_step_sched *rec, const double *lr_table, int64_t n_lr, const float *ema_table,
                              int64_t n_ema, void *stream);
/* tramba_adam_step_ctl with the record (sched == NULL && ema == NULL is tramba_adam_step_ctl bit for bit):
 *   sched: a device pointer.  The bias-corrected step size is formed in fp64 from lr * sched->lr_factor (a double product)
 *          instead of lr and nothing else changes: the call equals tramba_adam_step_ctl at lr' = lr * factor bit for bit,
 *          the factor read when the kernel runs.
 *   ema:   a HOST array of `count` device pointers, one fp32 tensor of the parameter's size each (needs sched).  After the
 *          parameter's update, in the same pass:  e = fmaf(w, p_new - e, e),  w = sched->ema_weight  (36 B per parameter
 *          instead of 28; the vector path when all five tensors are 16-byte aligned).  skip[0] != 0 leaves e as it is,
 *          with everything else.
 * 64 tensors per launch. */
int tramba_adam_step_sched(float *const *params, const float *const *grads, float *const *exp_avg, float *const *exp_avg_sq,
                           float *const *steps, const int64_t *numel, int count, double lr, double beta1, double beta2,
                           double eps, double weight_decay, const float *gscale, const int *skip, float *const *ema,
                           const tramba_step_sched *sched, void *stream);

/* ------------------------------------------------------------------ fused attention (Tramba-S / -P encoders, inference) */
/* Both entries: K and V of one (problem, head) are staged whole in LDS (at most 256 keys), scores on MFMA with f32
 * accumulation, scale = hd^-0.5 applied in f32 to the accumulated score, softmax in f32 with the row max subtracted, P
 * rounded to dtype only as the operand of P V, P V accumulated in f32, divided by the f32 row sum and rounded once.  No
 * atomics, fixed summation order (bitwise reproducible), no allocation or synchronisation (capturable).  bf16 / fp16 only,
 * hd = 32 or 64, tensors 16-byte aligned.  The query rows of one problem are dealt to several workgroups when the
 * (problem, head) pairs alone do not fill the chip. */
/* WindowAttention.forward with the cyclic shift, window_partition / window_reverse and the shift mask around it
 * (Models/encoder/swin_encoder.py:116-147, 213-232, 236-268).  qkv: (B, H, W, 3 C) as the qkv Linear writes it on the
 * unpermuted token map (channel order [3][heads][hd], C = heads * hd); table: ((2 ws - 1)^2, heads) f32, the module's
 * relative_position_bias_table; y: (B, H, W, C).  Window (wy, wx), local (i, j) is map position ((wy ws + i + shift) mod H,
 * (wx ws + j + shift) mod W), read and written there.  Bias index (i_q - i_k + ws - 1)(2 ws - 1) + (j_q - j_k + ws - 1).
 * shift > 0: rolled-frame rows / columns get a region 0 / 1 / 2 with cuts at H - ws and H - shift (W likewise), pair id
 * 3 r + c; query / key pairs of different id get -100 added (finite, as the reference).  No (nW, heads, N, N) tensor exists.
 * ws * ws <= 256, H % ws == 0, W % ws == 0, 0 <= shift < ws. */
int tramba_window_attn_cl(const void *qkv, const float *table, void *y, int batch, int h, int w, int heads, int hd,
                          int ws, int shift, int dtype, void *stream);
/* Attention.forward after its projections (Models/encoder/pvtv2_encoder.py:95-116): q (B, N, C), kv (B, M, 2 C) (channel
 * order [2][heads][hd]) -> y (B, N, C), all read and written in place through head strides; no bias.  1 <= M <= 256 (any M:
 * pad keys are kept out of the max, the sum and P), N >= 1. */
int tramba_kv_attn_cl(const void *q, const void *kv, void *y, int batch, int64_t n, int m, int heads, int hd, int dtype,
                      void *stream);

/* ------------------------------------------------------------------ attention backward (Tramba-S / -P encoders, training) */
/* Both forms, with S = hd^-0.5 Q K^T (+ bias + mask), P = softmax(S), dO the incoming gradient:
 *   dP = dO V^T,  D_q = sum_k P_qk dP_qk,  dS = P o (dP - D),  dV = P^T dO,  dQ = hd^-0.5 dS K,  dK = hd^-0.5 dS^T Q.
 * Nothing is saved by the forward: the row max and row sum are recomputed from q and k (at most 256 keys, K and V whole in
 * LDS).  Every product runs on MFMA with f32 accumulation; S, P, dP, D and dS stay in f32; hd^-0.5 multiplies accumulated
 * f32 values; 16-bit roundings happen only where P (for dV) and dS (for dQ / dK) become MFMA operands -- each as the pair
 * hi = round(x), lo = round(x - hi), two MFMAs, so that the products keep the f32 value -- and once at each output store.  No atomics and a fixed summation order (bitwise reproducible); no allocation or synchronisation
 * (capturable).  The caller allocates the workspace; its size is a pure function of the shape (tramba_*_attn_bwd_work,
 * 0 for a shape the entry refuses) and the entry checks what it is given against what it will use.  Arguments are
 * checked as by the forward entries; bf16 / fp16, hd 32 / 64, tensors 16-byte aligned. */
/* Backward of tramba_window_attn_cl, i.e. of WindowAttention.forward with the cyclic shift, window_partition /
 * window_reverse and the shift mask around it (Models/encoder/swin_encoder.py:116-147, 213-232, 236-268).  qkv, table
 * as the forward's; dy: (B, H, W, C); dqkv: (B, H, W, 3 C), written completely (every token lies in exactly one window:
 * no zero-fill, no accumulation), through the forward's shift arithmetic.  dtable: ((2 ws - 1)^2, heads) f32,
 * dtable[e, head] = sum of the f32 dS over batch, windows and the (q, k) pairs of relative index e: per-window sums in
 * query order, then windows in index order by a second launch.  dtable == NULL skips the table gradient and needs no
 * workspace (a frozen encoder). */
size_t tramba_window_attn_bwd_work(int batch, int h, int w, int heads, int hd, int ws);
int tramba_window_attn_bwd_cl(const void *qkv, const float *table, const void *dy, void *dqkv, float *dtable, void *work,
                              size_t work_bytes, int batch, int h, int w, int heads, int hd, int ws, int shift, int dtype,
                              void *stream);
/* Backward of tramba_kv_attn_cl, i.e. of Attention.forward after its projections (Models/encoder/pvtv2_encoder.py:95-116):
 * q (B, N, C), kv (B, M, 2 C), dy (B, N, C) -> dq (B, N, C), dkv (B, M, 2 C), read and written through head strides.  The N
 * queries of a (batch, head) are dealt to about 256 / heads workgroups in runs of 64-query rounds (32 above 160 keys); each writes f32 dK /
 * dV partials to the workspace and a second launch adds them in run order, scales dK and rounds once.  Rows of kv / dkv
 * beyond M are neither read nor written. */
size_t tramba_kv_attn_bwd_work(int batch, int64_t n, int m, int heads, int hd);
int tramba_kv_attn_bwd_cl(const void *q, const void *kv, const void *dy, void *dq, void *dkv, void *work, size_t work_bytes,
                          int batch, int64_t n, int m, int heads, int hd, int dtype, void *stream);

/* ------------------------------------------------------------------ dense convs of the Swin-B / PVTv2-b4 encoders (inference) */
/* Kernel = stride = r convolution on a channels-last map: the spatial-reduction conv `sr` of Attention.forward
 * (Models/encoder/pvtv2_encoder.py:76-78,103-106, with the permute / reshape around it).  x (B, Hin, Win, Cin) ->
 * y (B, Hin / r, Win / r, Cout), floor: trailing rows and columns of a map whose side is no multiple of r are never read.
 * w is K-major (Cout, r, r, Cin) = reference weight.permute(0,2,3,1), same dtype as x; bias (Cout) f32 or NULL.
 * bf16 / fp16, 2 <= r <= 8, Cin % 64 == 0, Cout % 8 == 0, tensors 16-byte aligned, the input map below 2^31 bytes.
 * f32 accumulation on the matrix cores with K split between the waves of a workgroup, the partial sums added in wave
 * order, one rounding; no atomics, no workspace, no allocation or synchronisation (capturable, bitwise reproducible). */
int tramba_patch_conv_cl(const void *x, const void *w, const float *bias, void *y, int batch, int hin, int win, int cin,
                         int cout, int r, int dtype, void *stream);
/* Backward of tramba_patch_conv_cl, i.e. of the `sr` conv of Attention.forward (Models/encoder/pvtv2_encoder.py:76-78,
 * 103-106) in 16-bit training.  Same domain as the forward: bf16 / fp16, 2 <= r <= 8, Cin % 64 == 0, Cout % 8 == 0, tensors
 * 16-byte aligned, every tensor below 2^31 bytes.  With token t = (b, i, j), M = B Ho Wo and k = (di r + dj) Cin + c:
 *
 * Input gradient: gx[b, i r + di, j r + dj, c] = sum_co gy[t, co] w[co, k], gy (B, Ho, Wo, Cout) and gx (B, Hin, Win, Cin) in
 * the activation dtype, w the forward's K-major (Cout, r, r, Cin) copy.  A GEMM over 16-token tiles reduced over Cout on the
 * matrix cores (the weight tile is staged as it lies and read transposed); one rounding; 16-byte stores into x's layout.
 * Every element of gx is written exactly once: rows >= r Ho and columns >= r Wo receive zeros. */
int tramba_patch_conv_dgrad_cl(const void *gy, const void *w, void *gx, int batch, int hin, int win, int cin, int cout, int r,
                               int dtype, void *stream);
/* Weight gradient: gw[co, k] = sum_t gy[t, co] x[patch(t), k] and, with want_bias, gb[co] = sum_t gy[t, co], f32, x read in
 * place.  The 32-token steps of the reduction are dealt in runs to S = tramba_patch_conv_wgrad_split(...) workgroups per
 * output tile (S depends on the shape alone; 0 for a shape the entry refuses).  `work` receives S slabs of
 * (Cout K + Cout) floats, slab z = [gw partial (Cout, r, r, Cin) | gb partial (Cout)] of run z; the gradient is their sum in
 * index order (tramba_slab_sum), and for S == 1 slab 0 is the gradient itself.  Without want_bias the gb part is
 * zero.  tramba_patch_conv_wgrad_work is the size of `work` in bytes.  No atomics: bitwise reproducible. */
int tramba_patch_conv_wgrad_split(int batch, int hin, int win, int cin, int cout, int r);
size_t tramba_patch_conv_wgrad_work(int batch, int hin, int win, int cin, int cout, int r);
int tramba_patch_conv_wgrad_cl(const void *gy, const void *x, float *work, size_t work_bytes, int batch, int hin, int win,
                               int cin, int cout, int r, int want_bias, int dtype, void *stream);
/* First-layer patch embedding fused with its LayerNorm: OverlapPatchEmbed.forward of patch_embed1
 * (Models/encoder/pvtv2_encoder.py:159-199; k 7 / stride 4 / pad 3, Cout 64) and PatchEmbed.forward
 * (Models/encoder/swin_encoder.py:413-450; k 4 / stride 4 / pad 0, Cout 128); any other form is refused.
 * img (B, 3, H, W) NCHW in f32 or `dtype`; w (Cout, 3, k, k) f32 reference layout; bias, ln_w, ln_b (Cout) f32;
 * y (B, Ho, Wo, Cout) bf16 / fp16, Ho = (H + 2 pad - k) / stride + 1 (floor).  Convolution, bias and LayerNorm in f32,
 * one rounding at the store (the reference rounds the convolution before the LayerNorm). */
int tramba_patch_embed_ln(const void *img, const float *w, const float *bias, const float *ln_w, const float *ln_b,
                          void *y, int batch, int h, int wd, int k, int stride, int pad, int cout, float eps,
                          int img_dtype, int dtype, void *stream);

/* ------------------------------------------------------------------ convolutions of the ResNet-50 encoder (inference) */
/* A bottleneck convolution with its eval-mode batch norm, shortcut and ReLU in one launch: conv1 / conv2 / conv3 of
 * Bottleneck.forward and the `downsample` branch (Models/encoder/resnet_encoder.py:62-110).  With t = (b, oi, oj) and
 * k = (di ksize + dj) Cin + c:
 *     y[t, co] = act( scale[co] * sum_k X[t, k] w[co, k] + shift[co] + residual[t, co] )
 * x (B, Hin, Win, Cin) channels-last; w K-major (Cout, ksize, ksize, Cin) = reference weight.permute(0,2,3,1), same dtype as
 * x and NOT rescaled; scale / shift (Cout) f32 or NULL (1 / 0), for a batch norm scale = gamma / sqrt(var + eps) and
 * shift = beta - mean * scale; residual (B, Ho, Wo, Cout) in dtype or NULL; relu 0 / 1; ksize 1 or 3, stride 1 or 2,
 * pad = ksize / 2, Ho = (Hin + 2 pad - ksize) / stride + 1.  bf16 / fp16, Cin % 64 == 0, Cout % 8 == 0, x / w / residual / y
 * 16-byte aligned, the input map below 2^31 bytes.  f32 accumulation on the matrix cores and an f32 epilogue, one rounding
 * at the store.  Two forms chosen from (M, K): waves own row blocks (tall maps), or the waves of a workgroup split K and
 * their partial sums are added in wave order (short, deep maps).  No atomics, no workspace, no allocation or
 * synchronisation (capturable, bitwise reproducible). */
int tramba_conv_affine_cl(const void *x, const void *w, const float *scale, const float *shift, const void *residual, void *y,
                          int batch, int hin, int win, int cin, int cout, int ksize, int stride, int relu, int dtype,
                          void *stream);
/* The ResNet stem: conv1 (7x7 / stride 2 / pad 3, 3 -> 64, no bias) + bn1 + ReLU + max_pool2d(3, 2, 1) of ResNet.forward
 * (Models/encoder/resnet_encoder.py:62-110).  img (B, 3, H, W) NCHW in f32 or `dtype`; w (64, 3, 7, 7) f32 reference layout;
 * scale / shift (64) f32 (the folded batch norm); y (B, Hp, Wp, 64) channels-last bf16 / fp16 with Hc = (H - 1) / 2 + 1,
 * Hp = (Hc - 1) / 2 + 1.  The half-resolution map is never written; the pool's padding is excluded from the max.
 * Convolution, affine and max in f32, one rounding at the store. */
int tramba_stem7_affine_relu_pool(const void *img, const float *w, const float *scale, const float *shift, void *y, int batch,
                                  int h, int wd, int img_dtype, int dtype, void *stream);

/* Backward of tramba_conv_affine_cl's convolution (scale / shift NULL, no ReLU: the raw convolution that the training path
 * hands to its batch norm), i.e. of conv1 / conv2 / conv3 / downsample[0] of Bottleneck.forward under autograd
 * (Models/encoder/resnet_encoder.py:62-110).  ksize 1 or 3, stride 1 or 2, pad = ksize / 2, bf16 / fp16, tensors 16-byte
 * aligned, every tensor below 2^31 bytes.  With t = (b, oi, oj), M = B Ho Wo and k = (di ksize + dj) Cin + c:
 *
 * Input gradient: gx[b, p, q, c] = sum over (di, dj, co) of gy[b, oi, oj, co] w[co, di, dj, c] where oi stride = p + pad - di
 * and oj stride = q + pad - dj have a solution inside the output map.  gy (B, Ho, Wo, Cout), gx (B, Hin, Win, Cin); wt is
 * the TRANSPOSED weight copy (Cin, ksize, ksize, Cout) = reference weight.permute(1,2,3,0), taps not mirrored.  Cout % 64 == 0
 * and Cin % 8 == 0; 1x1 / stride 1 is the plain product gy wt^T and runs on tramba_linear_cl (Cout % 8 == 0 there).  The
 * implicit GEMM of the forward over (tap, co) with its two forms; no zero-inserted map is built.  f32 accumulation, one
 * rounding; EVERY element of gx is written, pixels that no output reaches receive 0. */
int tramba_conv_dgrad_cl(const void *gy, const void *wt, void *gx, int batch, int hin, int win, int cin, int cout, int ksize,
                         int stride, int dtype, void *stream);
/* Weight gradient: gw[co, k] = sum_t gy[t, co] x[pixel(t, di, dj), c], f32 K-major (Cout, ksize, ksize, Cin), x read in place:
 * padding taps are predicated out, no column matrix is built, and the trailing pixels of x that a stride-2 convolution
 * never reaches are never read.  Cin % 64 == 0, Cout % 8 == 0.  The 32-token steps of the reduction are dealt in runs to
 * S = tramba_conv_wgrad_split(...) workgroups per output tile (S depends on the shape alone; 0 for a shape the entry
 * refuses).  `work` receives S slabs of Cout K floats; the gradient is their sum in index order (tramba_slab_sum), and for
 * S == 1 slab 0 is the gradient itself.  tramba_conv_wgrad_work is the size of `work` in bytes.  No atomics. */
int tramba_conv_wgrad_split(int batch, int hin, int win, int cin, int cout, int ksize, int stride);
size_t tramba_conv_wgrad_work(int batch, int hin, int win, int cin, int cout, int ksize, int stride);
int tramba_conv_wgrad_cl(const void *gy, const void *x, float *work, size_t work_bytes, int batch, int hin, int win, int cin,
                         int cout, int ksize, int stride, int dtype, void *stream);

/* ------------------------------------------------------------------ batch norm and max pool of the ResNet-50 encoder (training) */
/* Training-mode nn.BatchNorm2d (+ shortcut + ReLU) and the stem's max_pool2d(3, 2, 1) of Bottleneck.forward / ResNet.forward
 * (Models/encoder/resnet_encoder.py:62-110) on channels-last maps (M = B H W, C): bf16 / fp16, C % 8 == 0, maps 16-byte
 * aligned, f32 arithmetic, one rounding at a 16-bit store.  No atomics: every sum across workgroups goes through f32
 * partials of P = tramba_bn_parts(m, c) contiguous row runs in the caller's workspace of tramba_bn_work(m, c) bytes, added
 * in index order, so every result is a fixed function of the inputs (bitwise reproducible, capturable: no allocation, no
 * synchronisation).  The workspace holds 2 P + 2 rows of C rounded up to 64 floats and carries nothing between calls.
 *
 * Statistics: mean[c] = sum_t x[t, c] / M and rstd[c] = 1 / sqrt(var[c] + eps) with the biased variance
 * var[c] = sum_t (x[t, c] - mean[c])^2 / M, in two passes over x (never E[x^2] - E[x]^2).  running_mean / running_var (C) f32
 * or NULL: updated in place on the device, running = (1 - momentum) running + momentum new, where the new variance is the
 * unbiased var M / (M - 1).  M == 1 is refused, as F.batch_norm refuses it in training.  num_batches_tracked is the caller's. */
int tramba_bn_parts(int64_t m, int c);
size_t tramba_bn_work(int64_t m, int c);
int tramba_bn_stats_cl(const void *x, float *mean, float *rstd, float *running_mean, float *running_var, void *work,
                       size_t work_bytes, int64_t m, int c, float eps, float momentum, int dtype, void *stream);
/* y[t, c] = act( gamma[c] (x[t, c] - mean[c]) rstd[c] + beta[c] + residual[t, c] ).  gamma / beta (C) f32 or NULL (1 / 0);
 * residual (M, C) in dtype or NULL; relu 0 / 1. */
int tramba_bn_act_cl(const void *x, const float *mean, const float *rstd, const float *gamma, const float *beta,
                     const void *residual, void *y, int64_t m, int c, int relu, int dtype, void *stream);
/* Backward of tramba_bn_act_cl through the batch statistics.  With dy' = dy where y > 0 and 0 elsewhere (relu; y is read for
 * this mask alone and may be NULL without relu) and xh = (x - mean) rstd:
 *     dbeta[c] = sum_t dy'[t, c]      dgamma[c] = sum_t dy'[t, c] xh[t, c]
 *     dx[t, c] = gamma[c] rstd[c] ( dy'[t, c] - dbeta[c] / M - xh[t, c] dgamma[c] / M )      dres = dy'
 * dx (M, C) in dtype is always written; dres (M, C) in dtype, dgamma, dbeta (C) f32 may each be NULL (no shortcut; a frozen
 * affine, whose dx is bitwise the unfrozen one).  Three launches: partial sums per row run, their sum, dx. */
int tramba_bn_act_bwd_cl(const void *dy, const void *x, const void *y, const float *mean, const float *rstd, const float *gamma,
                         void *dx, void *dres, float *dgamma, float *dbeta, void *work, size_t work_bytes, int64_t m, int c,
                         int relu, int dtype, void *stream);
/* max_pool2d(kernel 3, stride 2, padding 1) on x (B, H, W, C) -> y (B, Ho, Wo, C), Ho = (H - 1) / 2 + 1.  Padding is never
 * looked at; among equal values the FIRST of the window in row-major order is the maximum, a NaN replaces it (the framework's
 * rule).  Backward in gather form: gx (B, H, W, C), every element written; an input pixel visits the at most 4 windows that
 * cover it, recomputes their arg-max from x and adds gy where it is the arg-max itself (f32, one rounding). */
int tramba_maxpool3s2_cl(const void *x, void *y, int batch, int h, int w, int c, int dtype, void *stream);
int tramba_maxpool3s2_bwd_cl(const void *gy, const void *x, void *gx, int batch, int h, int w, int c, int dtype, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* TRAMBA_HIP_H */
