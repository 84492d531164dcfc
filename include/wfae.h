/*
 * wfae.h — C ABI of libwfae.so: hand-written HIP/gfx950 kernels for the
 * conv-autoencoder training hot path of Autobot37/weatherforecastingtoolkit.
 *
 * The reference has NO native/FFI boundary (it is 100 % Python, every kernel
 * is a stock ATen op reached through torch.nn — SURVEY.md §0.1, §8b), so this
 * ABI is defined by the build.  Each entry point names the reference call
 * site whose ATen op it replaces (paths relative to the reference root).
 *
 * Conventions
 *   - all tensors are dense fp32, NCHW, caller-owned DEVICE pointers
 *     (torch: tensor.data_ptr()); the library never allocates, frees or
 *     retains device memory;
 *   - `ws`/`ws_bytes` is caller-provided scratch (query with
 *     wfae_workspace_bytes); contents are undefined after the call;
 *   - `stream` is a hipStream_t passed as void* (torch:
 *     torch.cuda.current_stream().cuda_stream); every launch goes to it, no
 *     implicit device synchronisation;
 *   - return 0 on success, a negative wfae_status otherwise; never throws or
 *     aborts; wfae_last_error_string() describes the calling thread's last
 *     failure;
 *   - re-entrant and thread-safe: no mutable global state except the
 *     matmul-precision mode below (one atomic int, set once at start-up);
 *   - `accumulate` != 0 means "out += result" (gradient accumulation),
 *     0 means "out = result".
 */
#ifndef WFAE_H
#define WFAE_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef void* wfae_stream_t;

typedef enum {
  WFAE_OK = 0,
  WFAE_ERR_BAD_SHAPE = -1,
  WFAE_ERR_NULL_POINTER = -2,
  WFAE_ERR_WORKSPACE = -3,
  WFAE_ERR_LAUNCH = -4,
  WFAE_ERR_UNSUPPORTED = -5
} wfae_status;

/* ABI history (wfae_version() = 100 * major + minor; a caller built against another minor must re-check the entry
 * points named here):
 *   100  round 1.
 *   101  wfae_conv1x1_fwd_stats / wfae_conv1x1_fwd_bnact / wfae_bn_stats_from_rows: `stat_part` changed from float* to
 *        double* and `stat_capacity` counts DOUBLES (the epilogue sums are reduced in fp64).  A caller built against 100
 *        would hand over a buffer of half the byte size: check wfae_version() >= 101 before using them.
 *   102  round 3: wfae_c1gemm_* (1x1 convolutions on the bf16 matrix pipe with exact split operands, fused BatchNorm
 *        backward epilogues), the bf16 ACTIVATION STORAGE entry points (*_bf16, *_bf16in, *_bf16out, wfae_convert_*),
 *        wfae_c1b_*, wfae_c1w_*, wfae_g3b_* added; nothing removed.
 *   103  round 4: REMOVED wfae_c1gemm_* (six entry points) and wfae_conv1x1_bwd_data_bnred / _bndx (the fused
 *        BatchNorm-backward epilogues of the tile-synchronous GEMMs: parity-green, never faster — the record is
 *        profiles/r03_kbench_c1_fused_bn_backward.txt); wfae_g3b_fwd no longer serves 8 channels per group;
 *        wfae_bn_act_bwd_from_rows now finishes the partial rows of wfae_c1r_bnred.  ADDED
 *        wfae_c1r_* (register-direct 1x1 convolutions: fp32 tensors, C <= 256 stages and the C >= 512 widening products;
 *        wfae_c1r_bnred / wfae_c1r_bndx: the BatchNorm backward of the layer in front in the data gradient's epilogue) and
 *        wfae_c1rb_* (the same on bf16-stored tensors, every stage). */
int wfae_version(void);
const char* wfae_last_error_string(void);
/* upper bound of scratch bytes any single call needs for a problem whose
 * largest weight tensor has `max_weight_elems` elements. */
size_t wfae_workspace_bytes(int64_t max_weight_elems);

/* ---- arithmetic mode of the MFMA GEMM family ------------------------------
 * counterpart of torch.set_float32_matmul_precision(...), which the reference
 * calls once at start-up (experiments/ae_v2/train.py:270, ae_v2_2/train.py:223)
 * and of BASELINE config 5 ("bf16").  WFAE_PRECISION_FP32 (default): operands
 * and accumulation in fp32 (v_mfma_f32_32x32x2_f32).  WFAE_PRECISION_BF16:
 * tensors stay fp32 in HBM; every GEMM-family kernel (1x1 / linear / 4x4 /
 * Winograd / flat-shift convolutions, all three roles) rounds its two operands
 * to bf16 (RNE) on the way from LDS to the matrix core and accumulates in fp32
 * (v_mfma_f32_32x32x16_bf16) — torch's 'medium'.  Process-wide; read at launch. */
enum { WFAE_PRECISION_FP32 = 0, WFAE_PRECISION_BF16 = 1 };
int wfae_set_matmul_precision(int mode);
int wfae_get_matmul_precision(void);

/* fp32 GEMMs on the bf16 matrix pipe ("split" operands, see the Winograd section below): at WFAE_PRECISION_FP32 the
 * MFMA-bound GEMMs carry every fp32 operand exactly as three bf16 values and multiply with six
 * v_mfma_f32_32x32x16_bf16 per fp32 product — fp32 accuracy at up to 16/6 of the fp32 instruction's rate.  On by
 * default (environment WFAE_SPLIT_GEMM=0 turns it off at load); 0 keeps every GEMM on v_mfma_f32_32x32x2_f32.
 * Process-wide; read at launch. */
int wfae_set_split_gemm(int on);
int wfae_get_split_gemm(void);

/* The narrowing 1x1 products of the C >= 512 Bottlenecks (wfae_conv1x1_fwd / _fwd_stats / _fwd_bnact without bias and
 * residual, and wfae_conv1x1_bwd_data, at (Cout, Cin) resp. (Cin, Cout) = (128, 512) or (256, 1024), HW % 8 == 0, 16-byte
 * aligned tensors, fp32 precision with the split GEMMs on) run on csrc/c1n.hip: both operands are split into their three
 * bf16 planes once, on their way into LDS.  On by default (environment WFAE_C1N=0 turns it off at load); 0 keeps these shapes on the in-register split of the generic
 * GEMM kernel (the A/B switch of tools/kbench.py and tests/test_c1n_gpu.py).  Process-wide; read at launch. */
int wfae_set_c1n(int on);
int wfae_get_c1n(void);

/* ---- 1x1 convolution as an fp32-MFMA GEMM on NCHW ------------------------
 * replaces nn.Conv2d(C, C/4, 1) / (C/4, C, 1) in Bottleneck
 * (pipeline/models/ae_64x8x8_lin.py:15,19) and the latent projections
 * enc[4] / dec[0] (:69,79).
 * y[n,co,p] = sum_ci w[co,ci] x[n,ci,p] (+ bias[co]) (+ res[n*res_img_stride + co*HW + p])
 * res_img_stride = Cout*HW for the Bottleneck residual (:22), 0 for the
 * broadcast pos_emb add (:91). */
int wfae_conv1x1_fwd(const float* x, const float* w, const float* bias, const float* res,
                     int64_t res_img_stride, float* y, int NB, int Cin, int Cout, int HW,
                     wfae_stream_t stream);
/* Same convolution with the BatchNorm statistics of y (the next layer of Bottleneck is always
 * BatchNorm2d, ae_64x8x8_lin.py:14-19) reduced in the epilogue instead of by a second pass over y:
 * stat_part (capacity stat_capacity DOUBLES) receives *stat_rows partial rows, sum[rows][Cout] followed by
 * sumsq[rows][Cout] (one row per 64-pixel wave tile, reduced in fp64 from fp32 sums of four — the arithmetic of the
 * separate statistics pass, so its results are reproduced to fp64 rounding); wfae_bn_stats_from_rows finishes them.  When the
 * shape is not served by the vector epilogue *stat_rows is 0: y is still complete, run
 * wfae_bn_stats_train on it.  stat_rows is a HOST pointer. */
int wfae_conv1x1_fwd_stats(const float* x, const float* w, const float* bias, const float* res,
                           int64_t res_img_stride, float* y, int NB, int Cin, int Cout, int HW,
                           double* stat_part, int64_t stat_capacity, int* stat_rows, wfae_stream_t stream);
/* BatchNorm-apply + GELU fused into the 1x1 GEMM's operand loader (SURVEY.md 2.2 K3/K7/K8 "fused prologue"):
 * y = conv1x1(gelu(x * bn_scale[c] + bn_shift[c]), w) (+bias)(+res) and, for the backward pass,
 * dw (+)= dy * gelu(x * bn_scale + bn_shift)^T — the activated tensor of the reference's BN -> GELU -> Conv1x1 chain
 * (pipeline/models/ae_64x8x8_lin.py:14-15) is rebuilt between the global load and the LDS store and never exists in
 * HBM.  bn_scale / bn_shift [Cin] are the folded vectors wfae_bn_stats_train / wfae_bn_fold_eval produce; results are
 * bit-identical to wfae_bn_act_fwd followed by wfae_conv1x1_fwd / wfae_conv1x1_bwd_weight (in either matmul precision).
 * HW % 4 == 0 (>= 16 for the weight gradient), channel counts % 4 == 0 and 16-byte aligned tensors only
 * (WFAE_ERR_UNSUPPORTED otherwise: run the two-kernel form). */
int wfae_conv1x1_fwd_bnact(const float* x, const float* bn_scale, const float* bn_shift, const float* w,
                           const float* bias, const float* res, int64_t res_img_stride, float* y, int NB, int Cin,
                           int Cout, int HW, double* stat_part, int64_t stat_capacity, int* stat_rows,
                           wfae_stream_t stream);   /* stat_part / stat_rows: as wfae_conv1x1_fwd_stats, or both null */
int wfae_conv1x1_bwd_weight_bnact(const float* dy, const float* x, const float* bn_scale, const float* bn_shift,
                                  float* dw, int NB, int Cin, int Cout, int HW, int accumulate, void* ws,
                                  size_t ws_bytes, wfae_stream_t stream);
int wfae_conv1x1_bwd_data(const float* dy, const float* w, float* dx, int NB, int Cin, int Cout,
                          int HW, wfae_stream_t stream);
int wfae_conv1x1_bwd_weight(const float* dy, const float* x, float* dw, int NB, int Cin, int Cout,
                            int HW, int accumulate, void* ws, size_t ws_bytes, wfae_stream_t stream);

/* ---- The Bottleneck's 1x1 convolutions at the HBM-bound stages, "register-direct" (csrc/c1r.hip, ABI 103).
 * Same products as wfae_conv1x1_fwd[_stats|_bnact] / wfae_conv1x1_bwd_data (pipeline/models/ae_64x8x8_lin.py:15,19):
 *   y[n,m,p] = sum_k A[m,k] f(x[n,k,p]) (+ res[n,m,p]),   A[m,k] = w[m * w_sm + k * w_sk]
 * (forward: M = Cout, K = Cin, w_sm = Cin, w_sk = 1; data gradient: M = Cin, K = Cout, w_sm = 1, w_sk = Cin — the same
 * (Cout, Cin) weight tensor either way).  fp32 tensors; every operand value is carried exactly as three bf16 values (six
 * v_mfma_f32_16x16x32_bf16 products per fp32 product, fp32 accumulation: the accuracy of the fp32 path, needs the split
 * GEMMs on).  The activation goes HBM -> registers -> matrix core with no LDS staging (16-byte loads of four pixels of eight
 * channel rows per lane; the four pixel components feed four MFMAs), results leave as 16-byte stores; the weights are split
 * by the kernel itself into an LDS image.  Served: (M, K) = (32, 128), (64, 256), (128, 32), (256, 64) — the C = 128 and
 * C = 256 stages — with HW % 64 == 0 (wfae_c1r_supported).
 *   pro_scale / pro_shift [K] non-null: f = GELU(x * scale[k] + shift[k]) (wfae_conv1x1_fwd_bnact's prologue), else identity;
 *   res non-null: residual add (M > K only);
 *   stat_part non-null: BatchNorm sums of y, *stat_rows = wfae_c1r_stat_rows(...) partial rows, sum[rows][M] then
 *   sumsq[rows][M] in fp64 (one row per wave of the persistent grid; finish with wfae_bn_stats_from_rows); capacity
 *   2 * rows * M doubles.  stat_rows is a HOST pointer. */
int wfae_c1r_supported(int M, int K, int HW);
int wfae_c1r_stat_rows(int M, int K, int NB, int HW);
int wfae_c1r_fwd(const float* w, int64_t w_sm, int64_t w_sk, const float* x, const float* pro_scale, const float* pro_shift,
                 const float* res, float* y, int NB, int K, int M, int HW, double* stat_part, int64_t stat_capacity,
                 int* stat_rows, wfae_stream_t stream);
/* The widening DATA GRADIENT of the C <= 256 stages with the reductions of the BatchNorm + GELU backward of the layer in front
 * taken in its epilogue (csrc/c1r.hip, ABI 103): da (NB,M,HW) = A dt as wfae_c1r_fwd, and part = sum dU [rows][M] then sum dU xhat
 * [rows][M] in fp64, dU = da * gelu'(x * bn_scale + bn_shift), xhat = (x - save_mean) * save_invstd, x (NB,M,HW) the BatchNorm
 * input — phase 1 of wfae_bn_act_bwd without its pass over (da, x); da may be NULL (the sums alone).  Finish with wfae_bn_act_bwd_from_rows (dgamma, dbeta and the
 * coefficients at the head of ws), then wfae_bn_act_bwd(phases = 2, same ws).  rows <= wfae_c1r_stat_rows(M, K, NB, HW). */
int wfae_c1r_bnred_supported(int M, int K, int HW);
int wfae_c1r_bnred(const float* w, int64_t w_sm, int64_t w_sk, const float* dt, const float* x, const float* bn_scale,
                   const float* bn_shift, const float* save_mean, const float* save_invstd, float* da, int NB, int K, int M, int HW,
                   double* part, int64_t part_capacity, int* part_rows, wfae_stream_t stream);
int wfae_bn_act_bwd_from_rows(const double* part, int rows, int C, float* dgamma, float* dbeta, int accumulate, void* ws,
                              size_t ws_bytes, wfae_stream_t stream);
/* The second pass of that backward in the epilogue of the SAME data gradient, computed again from dt (csrc/c1r.hip, ABI 103):
 *   dx (NB,M,HW) = gamma * save_invstd * (dU - coef[2c] / n - xhat * coef[2c+1] / n) + res,   n = NB * HW,
 * dU, xhat as above with da = A dt rebuilt in registers; coef = the two sums per channel that wfae_bn_act_bwd_from_rows leaves at
 * the head of its ws (training = 0: both taken as zero); res (the gradient arriving over the skip connection) may be null.  With
 * wfae_c1r_bnred(da = NULL) — the sums alone, nothing stored — the layer's backward moves dt twice and x twice, res and dx once,
 * where the da-storing sequence (wfae_c1r_bnred + wfae_bn_act_bwd phases = 2) also writes and re-reads da.  Replaces
 * wfae_bn_act_bwd(phases = 2) for the shapes of wfae_c1r_bnred_supported. */
int wfae_c1r_bndx(const float* w, int64_t w_sm, int64_t w_sk, const float* dt, const float* x, const float* gamma,
                  const float* bn_scale, const float* bn_shift, const float* save_mean, const float* save_invstd, const float* coef,
                  const float* res, float* dx, int NB, int K, int M, int HW, int training, wfae_stream_t stream);
/* The same register-direct product on bf16-STORED tensors (csrc/c1rb.hip, ABI 103; needs WFAE_PRECISION_BF16): bf16 pieces of
 * eight pixels per lane go HBM -> registers -> v_mfma_f32_16x16x32_bf16 with four byte-permutes per fragment and no other
 * arithmetic, the weight as one bf16 plane rounded by the kernel itself, fp32 accumulation, one rounding of the result.  Serves
 * every Bottleneck product (M, K) = (C/4, C) and (C, C/4), C = 128 .. 1024, with HW % 128 == 0 (wfae_c1rb_supported); other
 * shapes: wfae_c1b_fwd.  Arguments as wfae_c1r_fwd with uint16_t tensors; the BatchNorm sums are those of the ROUNDED result. */
int wfae_c1rb_supported(int M, int K, int HW);
int wfae_c1rb_stat_rows(int M, int K, int NB, int HW);
int wfae_c1rb_fwd(const float* w, int64_t w_sm, int64_t w_sk, const uint16_t* x, const float* pro_scale, const float* pro_shift,
                  const uint16_t* res, uint16_t* y, int NB, int K, int M, int HW, double* stat_part, int64_t stat_capacity,
                  int* stat_rows, wfae_stream_t stream);
/* Weight gradients of the Bottleneck's 1x1 convolutions with both operands read as K-contiguous rows (csrc/c1w.hip, ABI
 * 102): dw (Cout,Cin) (+)= dy (NB,Cout,HW) . x'^T, x' = x or (bn_scale / bn_shift non-null) gelu(x * bn_scale[c] +
 * bn_shift[c]) rebuilt in the loader (wfae_conv1x1_bwd_weight_bnact's prologue).  fp32 tensors: exact three-plane bf16
 * split at the LDS store, six bf16 MFMA products per fp32 product (needs the split GEMMs on); _bf16: bf16-stored tensors,
 * one product (needs WFAE_PRECISION_BF16).  HW % 32 == 0, channel counts % 32 == 0 (wfae_c1w_supported); ws holds the
 * split-K slabs: up to NB * ceil(HW / 256) slabs of Cout * Cin floats (fewer when they would not fit). */
int wfae_c1w_supported(int Cin, int Cout, int HW);
int wfae_c1w_bwd_weight(const float* dy, const float* x, const float* bn_scale, const float* bn_shift, float* dw, int NB, int Cin,
                        int Cout, int HW, int accumulate, void* ws, size_t ws_bytes, wfae_stream_t stream);
int wfae_c1w_bwd_weight_bf16(const uint16_t* dy, const uint16_t* x, const float* bn_scale, const float* bn_shift, float* dw, int NB,
                             int Cin, int Cout, int HW, int accumulate, void* ws, size_t ws_bytes, wfae_stream_t stream);
/* The two products of a Bottleneck's backward pass that read the incoming gradient dy (NB,C,HW) at C = 128 / 256, mid = C / 4,
 * in ONE pass over dy (csrc/c1wd.hip): dw3 (C,mid) (+)= dy . gelu(t2 * bn_scale[m] + bn_shift[m])^T — the result of
 * wfae_c1w_bwd_weight on the same arguments, bit for bit — and da3 (NB,mid,HW) = w3^T dy — the result of wfae_c1r_fwd with the
 * transposed weight, bit for bit.  fp32 tensors at fp32 precision with the split GEMMs on, HW % 64 == 0, dy and t2 16-byte
 * aligned; ws as wfae_c1w_bwd_weight.  wfae_c1wd_supported: 1 when the shape is served and the switch is on
 * (wfae_set_c1wd, on by default; environment WFAE_C1WD=0 turns it off at load) — otherwise wfae_c1wd_bwd returns
 * WFAE_ERR_UNSUPPORTED and the caller runs the two launches.  Process-wide; read at launch. */
int wfae_set_c1wd(int on);
int wfae_get_c1wd(void);
int wfae_c1wd_supported(int C, int mid, int HW);
int wfae_c1wd_bwd(const float* dy, const float* t2, const float* bn_scale, const float* bn_shift, const float* w3, float* dw3,
                  float* da3, int NB, int C, int mid, int HW, int accumulate, void* ws, size_t ws_bytes, wfae_stream_t stream);
/* The two passes of a Bottleneck's backward that read the block input x (NB,C,HW) in front of the first BatchNorm's sums at
 * C = 128 / 256, mid = C / 4, in ONE pass over x (csrc/c1ws.hip): dw1 (mid,C) (+)= dt1 . gelu(x * bn_scale[c] + bn_shift[c])^T —
 * the result of wfae_c1w_bwd_weight on the same arguments, bit for bit — and the partial rows of sum dU / sum dU xhat that
 * wfae_c1r_bnred(da = NULL) leaves (dU = (w1^T dt1) gelu'(x bn_scale + bn_shift); the same fp32 sums of four pixels, added in
 * fp64 in another order): `part` = [rows][C] ++ [rows][C] doubles, one row per workgroup, *part_rows = rows =
 * wfae_c1ws_stat_rows(C, mid, NB, HW, ws_bytes) (0: not served); finish with wfae_bn_act_bwd_from_rows.  fp32 tensors at fp32
 * precision with the split GEMMs on, HW % 64 == 0, x and dt1 16-byte aligned; ws as wfae_c1w_bwd_weight.
 * wfae_c1ws_supported: 1 when the shape is served and the switch is on (wfae_set_c1ws, on by default; environment WFAE_C1WS=0
 * turns it off at load) — otherwise wfae_c1ws_bwd returns WFAE_ERR_UNSUPPORTED and the caller runs the two launches.
 * Process-wide; read at launch. */
int wfae_set_c1ws(int on);
int wfae_get_c1ws(void);
int wfae_c1ws_supported(int C, int mid, int HW);
int wfae_c1ws_stat_rows(int C, int mid, int NB, int HW, size_t ws_bytes);
int wfae_c1ws_bwd(const float* x, const float* dt1, const float* bn_scale, const float* bn_shift, const float* save_mean,
                  const float* save_invstd, const float* w1, float* dw1, double* part, int64_t part_capacity, int* part_rows, int NB,
                  int C, int mid, int HW, int accumulate, void* ws, size_t ws_bytes, wfae_stream_t stream);
/* ---- nn.Linear (to_latent / from_latent, ae_64x8x8_lin.py:74-75,92,98) ---
 * y[b,o] = sum_i x[b,i] w[o,i] + bias[o] */
int wfae_linear_fwd(const float* x, const float* w, const float* bias, float* y, int B, int In,
                    int Out, void* ws, size_t ws_bytes, wfae_stream_t stream);
int wfae_linear_bwd_data(const float* dy, const float* w, float* dx, int B, int In, int Out,
                         wfae_stream_t stream);
int wfae_linear_bwd_weight(const float* dy, const float* x, float* dw, int B, int In, int Out,
                           int accumulate, wfae_stream_t stream);
/* the same with the batch dimension split across workgroups (deterministic slab reduce): for layers whose
 * Out x In tile grid is much smaller than the chip (transformer blocks) */
int wfae_linear_bwd_data_splitk(const float* dy, const float* w, float* dx, int B, int In, int Out, void* ws,
                                size_t ws_bytes, wfae_stream_t stream);
int wfae_linear_bwd_weight_splitk(const float* dy, const float* x, float* dw, int B, int In, int Out, int accumulate,
                                  void* ws, size_t ws_bytes, wfae_stream_t stream);

/* ---- 4x4 stride-2 pad-1 convolution pair ---------------------------------
 * "hi" = the 2H x 2W side with Chi channels, "lo" = the H x W side with Clo
 * channels.  Both nn.Conv2d(Chi, Clo, 4, 2, 1) weights (Clo,Chi,4,4)
 * (EncBlock.down[0], ae_64x8x8_lin.py:31) and nn.ConvTranspose2d(Clo, Chi, 4,
 * 2, 1) weights (Clo,Chi,4,4) (DecBlock.up[0], :42) are laid out
 * [lo][hi][ky][kx], so three kernels serve six operations:
 *   down : lo[n,l,oy,ox] = sum_{h,ky,kx} w[l,h,ky,kx] hi[n,h,2oy-1+ky,2ox-1+kx]
 *          = Conv2d forward            = ConvTranspose2d backward-data
 *   up   : hi[n,h,iy,ix] = sum_{l,ky,kx: iy=2oy-1+ky} w[l,h,ky,kx] lo[n,l,oy,ox]
 *          = ConvTranspose2d forward   = Conv2d backward-data
 *   wgrad: dw[l,h,ky,kx] = sum_{n,oy,ox} lo[n,l,oy,ox] hi[n,h,2oy-1+ky,2ox-1+kx]
 *          = Conv2d backward-weight (lo=dy, hi=x) = ConvTranspose2d
 *            backward-weight (lo=x, hi=dy)
 * Hlo,Wlo are the lo-side spatial dims. */
int wfae_conv4x4s2_down(const float* hi, const float* w, float* lo, int NB, int Chi, int Clo,
                        int Hlo, int Wlo, wfae_stream_t stream);
int wfae_conv4x4s2_up(const float* lo, const float* w, float* hi, int NB, int Chi, int Clo, int Hlo,
                      int Wlo, void* ws, size_t ws_bytes, wfae_stream_t stream);
int wfae_conv4x4s2_wgrad(const float* lo, const float* hi, float* dw, int NB, int Chi, int Clo,
                         int Hlo, int Wlo, int accumulate, void* ws, size_t ws_bytes,
                         wfae_stream_t stream);

/* ---- direct (im2col-free, LDS-tiled VALU) convolution ---------------------
 * grouped 3x3 pad 1 of Bottleneck (ae_64x8x8_lin.py:17), the 128->1 3x3 output
 * conv (:84) and the 1->256 4x4 s2 input conv (:31 with in_ch=1).
 * w is (Cout, Cin/groups, KS, KS).  (KS, stride) in {(3,1), (4,2), (4,1)}; (4,1) is the fourth conv of the
 * PatchGAN discriminator (losses/model.py:137).  bwd_data supports stride 1 only (H, W = input dims;
 * stride-2 data gradients go through wfae_conv4x4s2_up). */
int wfae_dconv_fwd(const float* x, const float* w, const float* bias, float* y, int NB, int Cin,
                   int Cout, int H, int W, int KS, int stride, int pad, int groups,
                   wfae_stream_t stream);
int wfae_dconv_bwd_data(const float* dy, const float* w, float* dx, int NB, int Cin, int Cout,
                        int H, int W, int KS, int pad, int groups, wfae_stream_t stream);
int wfae_dconv_bwd_weight(const float* dy, const float* x, float* dw, int NB, int Cin, int Cout,
                          int H, int W, int KS, int stride, int pad, int groups, int accumulate,
                          void* ws, size_t ws_bytes, wfae_stream_t stream);

/* grouped 3x3 pad-1 stride-1 convolution with Cin == Cout == C and C/groups in {4,8,16,32}
 * (the Bottleneck middle conv, ae_64x8x8_lin.py:17), register-blocked kernels.
 * fwd: transposed=0 -> y = conv(x, w); transposed=1 -> data gradient dx = conv^T(dy, w) (pass dy as x).
 * bwd_weight: dw[(g,oc),ci,ky,kx] as a per-group fp32-MFMA implicit GEMM over the pixels. */
int wfae_gconv3x3_fwd(const float* x, const float* w, float* y, int NB, int C, int H, int W, int groups,
                      int transposed, void* ws, size_t ws_bytes, wfae_stream_t stream);
int wfae_gconv3x3_bwd_weight(const float* dy, const float* x, float* dw, int NB, int C, int H, int W,
                             int groups, int accumulate, void* ws, size_t ws_bytes, wfae_stream_t stream);

/* ---- BatchNorm2d (+GELU) --------------------------------------------------
 * nn.BatchNorm2d(eps=1e-5, momentum=0.1) followed by nn.GELU()
 * (ae_64x8x8_lin.py:14,16,18,32,43).
 * bn_stats_train: per-channel batch mean / biased variance over (N,H,W)
 *   (fp64 accumulation), writes save_mean, save_invstd, the folded
 *   scale = gamma*invstd and shift = beta - mean*scale, and updates
 *   running_mean/var (unbiased var, momentum) in place.
 * bn_fold_eval: scale/shift from running statistics (module.eval()).
 * bn_act_fwd: y = act(x*scale[c] + shift[c]); act 0 = identity, 1 = exact GELU, 2 = LeakyReLU(0.2).
 * bn_act_bwd phases: 1 = per-channel reductions (+ dgamma/dbeta and the coefficients kept at the head of ws),
 *   2 = the dx kernel (reads those coefficients: same ws, no other call in between), 3 = both.
 * bn_act_bwd: given dy = dL/dy, x and the saved statistics, computes
 *   dgamma, dbeta and dx (+ res, the residual-branch gradient of
 *   Bottleneck, :22).  training=0 uses the eval-mode formula. */
int wfae_bn_stats_train(const float* x, int NB, int C, int HW, const float* gamma,
                        const float* beta, float eps, float momentum, float* running_mean,
                        float* running_var, float* save_mean, float* save_invstd, float* scale,
                        float* shift, void* ws, size_t ws_bytes, wfae_stream_t stream);
/* wfae_bn_stats_train's second half on the partial rows of wfae_conv1x1_fwd_stats (same outputs) */
int wfae_bn_stats_from_rows(const double* stat_part, int rows, int NB, int C, int HW, const float* gamma,
                            const float* beta, float eps, float momentum, float* running_mean,
                            float* running_var, float* save_mean, float* save_invstd, float* scale,
                            float* shift, void* ws, size_t ws_bytes, wfae_stream_t stream);
int wfae_bn_fold_eval(const float* gamma, const float* beta, const float* running_mean,
                      const float* running_var, float eps, float* save_mean, float* save_invstd,
                      float* scale, float* shift, int C, wfae_stream_t stream);
int wfae_bn_act_fwd(const float* x, const float* scale, const float* shift, float* y, int NB, int C,
                    int HW, int act, wfae_stream_t stream);
/* wfae_bn_act_fwd that also reduces the BatchNorm sums of ITS OUTPUT y (the first Bottleneck after a Down/Up unit
 * normalises y again): same fp64 partial layout as wfae_wino_out_stats, needs part_capacity >= 2 * C * NB * ceil(HW / 4096)
 * doubles.  wfae_bn_stats_from_parts = the second half of wfae_bn_stats_train (mean / invstd / folded scale, shift,
 * running-statistics update) on such partial sums; the sums are accumulated in fp64 like the separate pass, so the
 * statistics agree with it to fp64 rounding. */
int wfae_bn_act_fwd_stats(const float* x, const float* scale, const float* shift, float* y, int NB, int C, int HW, int act,
                          double* part, int64_t part_capacity, int* splits_out, wfae_stream_t stream);
int wfae_bn_stats_from_parts(const double* part, int splits, int NB, int C, int HW, const float* gamma, const float* beta,
                             float eps, float momentum, float* running_mean, float* running_var, float* save_mean,
                             float* save_invstd, float* scale, float* shift, wfae_stream_t stream);
int wfae_bn_act_bwd(const float* dy, const float* x, const float* gamma, const float* scale,
                    const float* shift, const float* save_mean, const float* save_invstd,
                    const float* res, float* dx, float* dgamma, float* dbeta, int NB, int C, int HW,
                    int act, int training, int accumulate, int phases, void* ws, size_t ws_bytes,
                    wfae_stream_t stream);

/* ---- bf16 ACTIVATION STORAGE (ABI 102; BASELINE config 5: the reference's bf16 regime, experiments/ae_v2_2/train.py:223
 * + Lightning precision).  In this mode the activation tensors of the convolution stacks — and their gradients — live in
 * HBM as bf16 bit patterns (torch.bfloat16, passed as uint16_t*), halving the traffic of the HBM-bound kernels; parameters,
 * parameter gradients, BatchNorm statistics, the latent vectors, the loss and every accumulation stay fp32, and each kernel
 * widens its inputs to fp32 registers and rounds results to nearest even on the way out.  A `_bf16` entry point is its
 * fp32 namesake with the activation pointers retyped; every lane still moves 16 bytes per access (8 elements instead
 * of 4), so HW % 8 == 0 takes the vector path (other sizes: the scalar path, as HW % 4 != 0 does for fp32). */
int wfae_convert_f32_to_bf16(const float* src, uint16_t* dst, int64_t n, wfae_stream_t stream);
int wfae_convert_bf16_to_f32(const uint16_t* src, float* dst, int64_t n, wfae_stream_t stream);
int wfae_bn_stats_train_bf16(const uint16_t* x, int NB, int C, int HW, const float* gamma, const float* beta, float eps,
                             float momentum, float* running_mean, float* running_var, float* save_mean, float* save_invstd,
                             float* scale, float* shift, void* ws, size_t ws_bytes, wfae_stream_t stream);
int wfae_bn_act_fwd_bf16(const uint16_t* x, const float* scale, const float* shift, uint16_t* y, int NB, int C, int HW, int act,
                         wfae_stream_t stream);
/* the sums are those of the ROUNDED values written to y (what the next BatchNorm reads) */
int wfae_bn_act_fwd_stats_bf16(const uint16_t* x, const float* scale, const float* shift, uint16_t* y, int NB, int C, int HW,
                               int act, double* part, int64_t part_capacity, int* splits_out, wfae_stream_t stream);
/* 1x1 convolutions on bf16-stored activations (x, res, y / dy, dx bf16; weights, bias, dw, BatchNorm vectors fp32; needs
 * WFAE_PRECISION_BF16; Cin % 4 == 0, HW % 4 == 0).  One entry point per role covers the plain and the fused forms:
 * bn_scale / bn_shift non-null = the BatchNorm + GELU prologue of wfae_conv1x1_fwd_bnact / wfae_conv1x1_bwd_weight_bnact,
 * stat_part / stat_rows non-null = the BatchNorm sums of wfae_conv1x1_fwd_stats (sums of the ROUNDED results). */
int wfae_conv1x1_fwd_bf16(const uint16_t* x, const float* bn_scale, const float* bn_shift, const float* w, const float* bias,
                          const uint16_t* res, int64_t res_img_stride, uint16_t* y, int NB, int Cin, int Cout, int HW,
                          double* stat_part, int64_t stat_capacity, int* stat_rows, wfae_stream_t stream);
int wfae_conv1x1_bwd_data_bf16(const uint16_t* dy, const float* w, uint16_t* dx, int NB, int Cin, int Cout, int HW,
                               wfae_stream_t stream);
int wfae_conv1x1_bwd_weight_bf16(const uint16_t* dy, const uint16_t* x, const float* bn_scale, const float* bn_shift, float* dw,
                                 int NB, int Cin, int Cout, int HW, int accumulate, void* ws, size_t ws_bytes,
                                 wfae_stream_t stream);
/* grouped 3x3 convolution of the Bottleneck on bf16-stored activations (weights / dw fp32) */
int wfae_gconv3x3_fwd_bf16(const uint16_t* x, const float* w, uint16_t* y, int NB, int C, int H, int W, int groups,
                           int transposed, void* ws, size_t ws_bytes, wfae_stream_t stream);
int wfae_gconv3x3_bwd_weight_bf16(const uint16_t* dy, const uint16_t* x, float* dw, int NB, int C, int H, int W, int groups,
                                  int accumulate, void* ws, size_t ws_bytes, wfae_stream_t stream);
/* the two full-resolution convolutions with ONE channel on one side keep that side fp32:
 *   dconv_fwd_bf16out:      Conv2d(1, C, 4, 2, 1) forward (encoder first layer): x fp32 (NB,1,H,W) -> y bf16 (NB,C,H/2,W/2)
 *   dconv_fwd_bf16in:       Conv2d(Cin, Cout, 3, 1, 1) forward (the output convolution): x bf16 -> y fp32
 *   dconv_bwd_data_bf16out: data gradient of Conv2d(Cin, 1, 3, 1, 1): dy fp32 (NB,1,H,W) -> dx bf16 (NB,Cin,H,W)
 *   c1_wgrad_bf16:          their weight gradients; flip 0: big = dy bf16 (NB,C,H/2,W/2), small = x fp32 (NB,1,H,W) -> dw
 *                           (C,1,4,4); flip 1: big = x bf16 (NB,C,H,W), small = dy fp32 (NB,1,H,W) -> dw (1,C,3,3) */
int wfae_dconv_fwd_bf16out(const float* x, const float* w, const float* bias, uint16_t* y, int NB, int Cout, int H, int W,
                           wfae_stream_t stream);
int wfae_dconv_fwd_bf16in(const uint16_t* x, const float* w, const float* bias, float* y, int NB, int Cin, int Cout, int H,
                          int W, wfae_stream_t stream);
int wfae_dconv_bwd_data_bf16out(const float* dy, const float* w, uint16_t* dx, int NB, int Cin, int H, int W,
                                wfae_stream_t stream);
int wfae_c1_wgrad_bf16(int flip, const uint16_t* big, const float* small, float* dw, int NB, int C, int H, int W, int accumulate,
                       void* ws, size_t ws_bytes, wfae_stream_t stream);
/* Winograd transforms with the TENSOR side stored as bf16 (operands / products of the transform domain unchanged);
 * wino_out_bf16 / wino_in_t_bf16: part null = plain transform, else also the BatchNorm sums of the rounded result */
int wfae_wino_in_split_bf16(int variant, const uint16_t* hi, uint16_t* V3, int planes, int NB, int Chi, int Hlo, int Wlo,
                            wfae_stream_t stream);
int wfae_wino_out_t_split_bf16(int variant, const uint16_t* lo, uint16_t* Mt3, int planes, int NB, int Clo, int Hlo, int Wlo,
                               wfae_stream_t stream);
int wfae_wino_out_bf16(int variant, const float* M, uint16_t* lo, int NB, int Clo, int Hlo, int Wlo, double* part,
                       int64_t part_capacity, int* splits_out, wfae_stream_t stream);
int wfae_wino_in_t_bf16(int variant, const float* dV, uint16_t* hi, int NB, int Chi, int Hlo, int Wlo, double* part,
                        int64_t part_capacity, int* splits_out, wfae_stream_t stream);
/* The Bottleneck's 1x1 convolutions on bf16-stored activations without a format change between HBM and the matrix core
 * (csrc/c1b.hip): y (bf16) = W f(x) (+ res), W one bf16 plane.  c1b_weights: w (Cout,Cin) fp32 -> Wb [Cout][Cin] and Wtb
 * [Cin][Cout] bf16 (the forward passes Wb with (M, K) = (Cout, Cin), the data gradient Wtb with (M, K) = (Cin, Cout)).
 * c1b_fwd: pro_scale / pro_shift [K] non-null = the BatchNorm + GELU prologue; stat_part non-null = BatchNorm sums of the
 * rounded y as *stat_rows rows, sum[rows][M] then sumsq[rows][M], rows = wfae_c1b_stat_rows(M, K, NB, HW), finish with
 * wfae_bn_stats_from_rows.  Served: M % 32 == 0, K % 32 == 0, HW % 8 == 0 (wfae_c1b_supported), WFAE_PRECISION_BF16 arithmetic. */
int wfae_c1b_supported(int M, int K, int HW);
int wfae_c1b_stat_rows(int M, int K, int NB, int HW);
int wfae_c1b_weights(const float* w, uint16_t* Wb, uint16_t* Wtb, int Cout, int Cin, wfae_stream_t stream);
int wfae_c1b_fwd(const uint16_t* Wb, const uint16_t* x, const float* pro_scale, const float* pro_shift, const uint16_t* res,
                 uint16_t* y, int NB, int K, int M, int HW, double* stat_part, int64_t stat_capacity, int* stat_rows,
                 wfae_stream_t stream);
/* The Bottleneck's grouped 3x3 convolution on bf16-stored activations as an implicit GEMM on the bf16 matrix pipe
 * (csrc/g3b.hip; reference pipeline/models/ae_64x8x8_lin.py:17): same arguments and result as wfae_gconv3x3_fwd_bf16 (which
 * routes here when wfae_g3b_supported says 1), transposed = 1 gives the data gradient.  Served: (channels per group, W) =
 * (4,384), (8,192), (16,96), (32,48), (32,24) with H a multiple of the strip height; workspace >= C/16 * 3 * 2 * 1024 bytes
 * (C/32 * 3 * 3 * 2 * 1024 at 32 channels per group) for the weight fragments.  WFAE_PRECISION_BF16 arithmetic. */
int wfae_g3b_supported(int C, int H, int W, int groups);
int wfae_g3b_fwd_bf16(const uint16_t* x, const float* w, uint16_t* y, int NB, int C, int H, int W, int groups, int transposed,
                      void* ws, size_t ws_bytes, wfae_stream_t stream);
/* weight gradient of the same convolution on the same kernel family (both tensors staged as they lie in memory, the kx shift
 * of a tap taken on the dy fragment in registers): dw (C, C/groups, 3, 3) fp32, += when accumulate; workspace >=
 * NB * (H / strip height) * C * (C/groups) * 9 * 4 bytes (one partial per block, added in fixed order) */
int wfae_g3b_bwd_weight_bf16(const uint16_t* dy, const uint16_t* x, float* dw, int NB, int C, int H, int W, int groups,
                             int accumulate, void* ws, size_t ws_bytes, wfae_stream_t stream);
/* the same kernels on fp32 tensors: every value split exactly into three bf16 planes at the LDS store, six products per fp32
 * product (the arithmetic of the split GEMMs: fp32 accuracy).  wfae_g3b_f32_supported(…, wgrad): 1 when the shape is served at
 * the current mode (fp32 precision with the split switch on; weight gradient at W <= 96 only: three planes of full-width rows exceed
 * the LDS at W = 384 and allow one block per CU at W = 192, which measured slower than wfae_gconv3x3_bwd_weight's kernel). */
int wfae_g3b_f32_supported(int C, int H, int W, int groups, int wgrad);
/* forward (transposed = 0) / data gradient (1) on fp32 tensors: (channels per group, W) = (16, 96) is what
 * wfae_g3b_f32_supported(…, 0) reports (faster than wfae_gconv3x3_fwd's kernel there); (8, 192) is accepted as well but measured
 * slower.  Same arguments as wfae_gconv3x3_fwd; workspace >= 3 x the bf16 form's */
int wfae_g3b_fwd(const float* x, const float* w, float* y, int NB, int C, int H, int W, int groups, int transposed, void* ws,
                 size_t ws_bytes, wfae_stream_t stream);
int wfae_g3b_bwd_weight(const float* dy, const float* x, float* dw, int NB, int C, int H, int W, int groups, int accumulate,
                        void* ws, size_t ws_bytes, wfae_stream_t stream);
int wfae_bn_act_bwd_bf16(const uint16_t* dy, const uint16_t* x, const float* gamma, const float* scale, const float* shift,
                         const float* save_mean, const float* save_invstd, const uint16_t* res, uint16_t* dx, float* dgamma,
                         float* dbeta, int NB, int C, int HW, int act, int training, int accumulate, int phases, void* ws,
                         size_t ws_bytes, wfae_stream_t stream);

/* ---- element-wise / reductions -------------------------------------------- */
int wfae_gelu_fwd(const float* x, float* y, int64_t n, wfae_stream_t stream);   /* nn.GELU */
int wfae_gelu_bwd(const float* dy, const float* x, float* dx, int64_t n, wfae_stream_t stream);
int wfae_sigmoid_fwd(const float* x, float* y, int64_t n, wfae_stream_t stream); /* :86,102 */
int wfae_sigmoid_bwd(const float* dy, const float* y, float* dx, int64_t n, wfae_stream_t stream);
int wfae_add(const float* a, const float* b, float* out, int64_t n, wfae_stream_t stream);
/* out[c] (+)= sum_{o,i} x[o,c,i]: conv-bias / pos_emb / linear-bias gradients */
int wfae_reduce_sum(const float* x, int outer, int C, int inner, float* out, int accumulate,
                    void* ws, size_t ws_bytes, wfae_stream_t stream);

/* ---- Winograd forms of the three 4x4 stride-2 operations above (same tensors, same results up to fp32
 * rounding).  The convolution is split into its four input-parity phases (each a 2x2 stride-1 convolution) and
 * every phase goes through F(MxM, 2x2) on N x N input tiles, N = M + 1:
 *   variant 0: F(2x2,2x2), 9 GEMMs,  18   FLOP per (lo channel, hi channel, lo pixel) instead of 32;
 *   variant 1: F(4x4,2x2), 25 GEMMs, 12.5 FLOP; interpolation points {0, +-1, +-2}.
 * xi = N*N transform positions, T = NB*Hlo*Wlo/M^2 tiles.  The pieces are separate entry points so that a
 * training step transforms every tensor once and reuses it (the weight gradient shares both transformed
 * operands with the forward / data gradient of the same layer):
 *   wino_weights:    w (Clo,Chi,4,4)       -> U  [xi][Clo][4Chi]   (G g G^T per phase)
 *   wino_in:         hi (NB,Chi,2Hlo,2Wlo) -> V  [xi][4Chi][T]     (B^T d B of the 2N x 2N patches at stride 2M)
 *   wino_out_t:      lo (NB,Clo,Hlo,Wlo)   -> Mt [xi][Clo][T]      (adjoint of the output transform)
 *   wino_gemm_down:  M  = U * V    [xi][Clo][T]   then  wino_out:  lo = A^T M A           (= wfae_conv4x4s2_down)
 *   wino_gemm_up:    dV = U^T * Mt [xi][4Chi][T]  then  wino_in_t: hi = overlap-add B dV B^T (= wfae_conv4x4s2_up)
 *   wino_gemm_wgrad: dw = G^T (Mt * V^T) G,  ws >= 2 * 4*|U| bytes                        (= wfae_conv4x4s2_wgrad)
 * with Mt = wino_out_t(lo-side tensor), V = wino_in(hi-side tensor).  Supported when Hlo, Wlo are multiples of
 * M, Chi % 4 == 0, Clo % 4 == 0 and T % 4 == 0; wfae_wino_sizes returns WFAE_ERR_UNSUPPORTED otherwise and
 * {T, |U|, |V|, |M|} (element counts) in out4 when it is. */
int wfae_wino_sizes(int variant, int NB, int Chi, int Clo, int Hlo, int Wlo, int64_t* out4);
int wfae_wino_weights(int variant, const float* w, float* U, int Chi, int Clo, wfae_stream_t stream);
int wfae_wino_in(int variant, const float* hi, float* V, int NB, int Chi, int Hlo, int Wlo, wfae_stream_t stream);
int wfae_wino_in_t(int variant, const float* dV, float* hi, int NB, int Chi, int Hlo, int Wlo, wfae_stream_t stream);
int wfae_wino_out(int variant, const float* M, float* lo, int NB, int Clo, int Hlo, int Wlo, wfae_stream_t stream);
/* wfae_wino_out that also reduces the BatchNorm sums of its result (the BatchNorm of EncBlock.down / DecBlock.up follows
 * the convolution directly, reference ae_64x8x8_lin.py:31-32,42-43): fp64 partial sums part[(split * Clo + c) * 2 +
 * {0 = sum, 1 = sum of squares}], *splits_out rows; finish them with wfae_bn_stats_from_parts. */
int wfae_wino_out_stats(int variant, const float* M, float* lo, int NB, int Clo, int Hlo, int Wlo, double* part,
                        int64_t part_capacity, int* splits_out, wfae_stream_t stream);
/* the same for the adjoint input transform, whose result is the output of a ConvTranspose2d (DecBlock.up, :42-43) */
int wfae_wino_in_t_stats(int variant, const float* dV, float* hi, int NB, int Chi, int Hlo, int Wlo, double* part,
                         int64_t part_capacity, int* splits_out, wfae_stream_t stream);
int wfae_wino_out_t(int variant, const float* lo, float* Mt, int NB, int Clo, int Hlo, int Wlo, wfae_stream_t stream);
int wfae_wino_gemm_down(int variant, const float* U, const float* V, float* M, int NB, int Chi, int Clo, int Hlo, int Wlo,
                        wfae_stream_t stream);
int wfae_wino_gemm_up(int variant, const float* U, const float* Mt, float* dV, int NB, int Chi, int Clo, int Hlo, int Wlo,
                      wfae_stream_t stream);
int wfae_wino_gemm_wgrad(int variant, const float* Mt, const float* V, float* dw, int NB, int Chi, int Clo, int Hlo,
                         int Wlo, int accumulate, void* ws, size_t ws_bytes, wfae_stream_t stream);

/* ---- The three Winograd-domain products on the bf16 matrix pipe at fp32 accuracy ("split" operands).
 * v_mfma_f32_32x32x2_f32 runs at the fp32 vector rate; v_mfma_f32_32x32x16_bf16 at 16x that.  An fp32 value is
 * exactly h + m + l with three bf16 values (h = bf16(x), m = bf16(x - h), l = bf16(x - h - m)) and bf16 x bf16 is exact
 * in fp32, so the six products ah bh, ah bm, am bh, ah bl, al bh, am bm accumulated in fp32 carry the fp32 product to
 * 2^-23 relative — the error of the fp32 MFMA path (tests/test_kernels_gpu.py::test_split_gemm_matches_fp32_accuracy) at
 * 16/6 of its rate.  A split operand is three planes of bf16 bit patterns (uint16_t), the h plane first, each plane
 * the fp32 layout's element count long; the *_split transforms write them directly (6 bytes per element instead of 4),
 * the GEMM outputs stay fp32 and go through wino_out / wino_in_t / the G^T dU G reduction unchanged.
 *   wino_weights_split: U3 [3][xi][Clo][4Chi] and Ut3 [3][xi][4Chi][Clo] (the up product contracts over Clo)
 *   wino_in_split / wino_out_t_split: V3 [3][xi][4Chi][T], Mt3 [3][xi][Clo][T]
 * Range: the split is exact for |x| in [2^-110, 3.3e38) (below, the l plane loses bits to bf16's underflow — the absolute
 * error stays under 2^-133; above, bf16(x) rounds to infinity); NaN and infinities propagate as NaN.
 * `planes` = 3: the exact split above.  `planes` = 1: only the h plane is written / read — bf16-rounded operands with
 * fp32 accumulation, i.e. WFAE_PRECISION_BF16's arithmetic with 2-byte operand storage for the matrix work (one MFMA
 * product per tile; the GEMMs turn HBM-bound).  Buffers hold `planes` planes.
 * wfae_wino_split_supported: 1 when wfae_wino_sizes accepts the geometry and 4 Chi, Clo and T are multiples of 32.
 * wfae_split_bf16x3 / wfae_split_gemm: the conversion and the batched product on their own (C[y] = A[y] B[y], A [M][K];
 * b_kind 0: B [K][N], b_kind 1: B [N][K]; K % 32 == 0, N % 8 == 0 for b_kind 0; planes batches*M*K resp. batches*K*N
 * elements apart). */
int wfae_wino_split_supported(int variant, int NB, int Chi, int Clo, int Hlo, int Wlo);
int wfae_wino_weights_split(int variant, const float* w, uint16_t* U3, uint16_t* Ut3, int planes, int Chi, int Clo,
                            wfae_stream_t stream);
int wfae_wino_in_split(int variant, const float* hi, uint16_t* V3, int planes, int NB, int Chi, int Hlo, int Wlo,
                       wfae_stream_t stream);
int wfae_wino_out_t_split(int variant, const float* lo, uint16_t* Mt3, int planes, int NB, int Clo, int Hlo, int Wlo,
                          wfae_stream_t stream);
int wfae_wino_gemm_down_split(int variant, const uint16_t* U3, const uint16_t* V3, float* M, int planes, int NB, int Chi, int Clo,
                              int Hlo, int Wlo, wfae_stream_t stream);
int wfae_wino_gemm_up_split(int variant, const uint16_t* Ut3, const uint16_t* Mt3, float* dV, int planes, int NB, int Chi, int Clo,
                            int Hlo, int Wlo, wfae_stream_t stream);
int wfae_wino_gemm_wgrad_split(int variant, const uint16_t* Mt3, const uint16_t* V3, float* dw, int planes, int NB, int Chi,
                               int Clo, int Hlo, int Wlo, int accumulate, void* ws, size_t ws_bytes, wfae_stream_t stream);
int wfae_split_bf16x3(const float* x, uint16_t* out, int64_t n, int planes, wfae_stream_t stream);
int wfae_split_gemm(int b_kind, int planes, const uint16_t* A3, const uint16_t* B3, float* C, int M, int N, int K, int batches,
                    wfae_stream_t stream);

/* ---- 4x4 stride-1 convolution on the MFMA GEMM (PatchGAN layer 4: Conv2d(256, 512, 4, stride=1, padding=1,
 * bias=False), pipeline/models/autoencoderkl/losses/model.py:137).
 * fwd, transposed = 0: x (NB,Cin,H,W) -> y (NB,Cout,H+2pad-3,W+2pad-3);
 * fwd, transposed = 1: the data gradient — x is dy (NB,Cout,H,W) -> y = dx (NB,Cin,H+3-2pad,W+3-2pad).
 * bwd_weight: dy (NB,Cout,H+2pad-3,W+2pad-3), x (NB,Cin,H,W) -> dw (Cout,Cin,4,4).
 * The channel count of the operand that is read must be a multiple of 16 (else WFAE_ERR_UNSUPPORTED; use
 * wfae_dconv_*).  Workspace: padded copy of the input + padded-width output + packed weights
 * (+ split-K slabs for bwd_weight). */
int wfae_conv4x4s1_fwd(const float* x, const float* w, float* y, int NB, int Cin, int Cout, int H, int W, int pad,
                       int transposed, void* ws, size_t ws_bytes, wfae_stream_t stream);
int wfae_conv4x4s1_bwd_weight(const float* dy, const float* x, float* dw, int NB, int Cin, int Cout, int H, int W,
                              int pad, int accumulate, void* ws, size_t ws_bytes, wfae_stream_t stream);

/* ---- PatchGAN discriminator pieces (pipeline/models/autoencoderkl/losses/model.py:100-150;
 * hinge loss contperceptual.py:19-23; generator term -mean(D(fake)) experiments/ae_v2/train.py:78).
 * leaky_relu: nn.LeakyReLU(0.2).  BatchNorm + LeakyReLU is wfae_bn_act_* with act = 2.
 * pad2d: zero-pad every plane by `pad` pixels (crop = 1: the inverse crop, its gradient) — the final
 *   Conv2d(512, 1, kernel_size=1, padding=1) of the reference is pad + 1x1 conv.
 * mean: out[0] = weight * mean(x) (hinge = 0) or weight * mean(relu(1 + sign*x)) (hinge = 1).
 * scale: y = x * scale * (scale_dev ? scale_dev[0] : 1)  (adaptive weight, gradient clipping). */
int wfae_leaky_relu_fwd(const float* x, float* y, int64_t n, wfae_stream_t stream);
int wfae_leaky_relu_bwd(const float* dy, const float* x, float* dx, int64_t n, wfae_stream_t stream);
int wfae_pad2d(const float* x, float* y, int64_t planes, int H, int W, int pad, int crop, wfae_stream_t stream);
int wfae_mean_fwd(const float* x, float* out, int64_t n, int hinge, float sign, float weight, void* ws,
                  size_t ws_bytes, wfae_stream_t stream);
int wfae_mean_bwd(const float* x, const float* gout, float* dx, int64_t n, int hinge, float sign, float weight,
                  wfae_stream_t stream);
int wfae_scale(const float* x, const float* scale_dev, float scale, float* y, int64_t n, wfae_stream_t stream);
/* gradient clipping by global norm (Lightning clip_gradients -> torch.nn.utils.clip_grad_norm_,
 * experiments/ae_v2_2/train.py:140,155): sumsq_parts are wfae_sumsq results of the gradient buffers;
 * total = pre_scale * sqrt(sum) (pre_scale = 1/world when the buffers hold rank-summed gradients);
 * out2[0] = min(1, max_norm / (total + 1e-6)), out2[1] = total; apply with wfae_scale(scale_dev = out2). */
int wfae_clip_coef(const double* sumsq_parts, int n_parts, float max_norm, float pre_scale, float* out2,
                   wfae_stream_t stream);
/* Loss.calculate_adaptive_weight (experiments/ae_v2_2/train.py:46-52, ae_v2/train.py:46-52):
 * out[0] = clamp(disc_weight * sqrt(sumsq_rec) / (sqrt(sumsq_disc) + 1e-4), 0, 1e4). */
int wfae_adaptive_weight(const double* sumsq_rec, const double* sumsq_disc, float disc_weight, float* out,
                         wfae_stream_t stream);

/* ---- Path-B latent linear forecaster (reference
 * experiments/v1_experiments/pretrained_ae_linear_sevir/train.py:67 `nn.Linear(T_in*C, T_out*C)` per latent pixel,
 * :73-83 training_step).  v is the latent sequence (B,T,C,H*W).
 * latent_diff_pack: X (B*HW, Tin*C)[t*C+c] = v[b,t,c,p] - v[b,Tin-1,c,p]  (the reference's `inp - inp_t` followed
 *   by permute(0,3,4,1,2).reshape(b,h,w,Tin*C), :77-81), Y (B*HW, Tout*C) = the same for the target frames (:78).
 *   The linear layer itself is wfae_linear_fwd / _bwd_weight on X.
 * latent_unpack_add: out (B,Tout,C,HW) = pred (B*HW, Tout*C) re-laid out + last input frame (`pred + inp_t`, :87).
 * mse: loss = mean((pred - target)^2) (F.mse_loss, :82), dpred = gloss * 2 (pred - target) / n. */
int wfae_latent_diff_pack(const float* v, float* X, float* Y, int B, int T, int Tin, int C, int HW,
                          wfae_stream_t stream);
int wfae_latent_unpack_add(const float* pred, const float* v, float* out, int B, int T, int Tin, int C, int HW,
                           wfae_stream_t stream);
int wfae_mse_fwd(const float* pred, const float* target, float* loss, int64_t n, void* ws, size_t ws_bytes,
                 wfae_stream_t stream);
int wfae_mse_bwd(const float* pred, const float* target, const float* gloss, float* dpred, int64_t n,
                 wfae_stream_t stream);

/* ---- DLinear latent forecasters (reference experiments/v1_experiments/
 * pretrained_ae_dlinear_{sevir,ind,indc_indp}/train.py:22-100 `moving_avg`, `series_decomp`, `DLinear`).
 * v (B, R, M): R rows per batch element, M columns; the predictor reads rows [0, L).  diff != 0 first subtracts the
 *   last input frame: row r -> row r - row (L - cf + r % cf) (`inp - inp_t`, cf = features per time step).
 * Decomposition along L with replicate padding of (K-1)/2 rows at each end: trend = AvgPool1d(K, stride 1),
 *   seasonal = x - trend.  K must be odd (K > L allowed).
 * dlinear_fwd: y (B, P, M) = Ws seasonal + bs + Wt trend + bt per column; individual != 0: W (M, P, L), b (M, P),
 *   else W (P, L), b (P) shared by all columns.
 * dlinear_bwd_weight: dWs = sum_b dy (x) seasonal, dWt likewise with trend, dbs = dbt = sum_b dy (summed over the
 *   columns too for shared weights: block partials + a fixed-order finalize, ws >= ceil(M/64) (2PL+P) floats).
 *   Outputs are overwritten; results are bitwise repeatable.
 * dlinear_bwd_data: dv (B, R, M) through the transposed decomposition (and the differencing); rows >= L are zero.
 *   ws >= 2 B L M floats.
 * series_decomp_fwd / _bwd: x (B, L, M) <-> (seasonal, trend).
 * dlinear_frames: mode 0 (target) out (B, P, M) = v[:, L + p] - v[:, L - cf + p % cf] (R >= L + P);
 *   mode 1 (forecast) out = a + v[:, L - cf + p % cf]  (`pred + inp_t`, the (B, Tout, C, h, w) latent layout). */
int wfae_dlinear_fwd(const float* v, const float* w_seasonal, const float* b_seasonal, const float* w_trend,
                     const float* b_trend, float* y, int B, int R, int M, int L, int P, int K, int individual, int diff,
                     int cf, wfae_stream_t stream);
int wfae_dlinear_bwd_weight(const float* v, const float* dy, float* dw_seasonal, float* db_seasonal, float* dw_trend,
                            float* db_trend, int B, int R, int M, int L, int P, int K, int individual, int diff, int cf,
                            void* ws, size_t ws_bytes, wfae_stream_t stream);
int wfae_dlinear_bwd_data(const float* dy, const float* w_seasonal, const float* w_trend, float* dv, int B, int R,
                          int M, int L, int P, int K, int individual, int diff, int cf, void* ws, size_t ws_bytes,
                          wfae_stream_t stream);
int wfae_series_decomp_fwd(const float* x, float* seasonal, float* trend, int B, int L, int M, int K,
                           wfae_stream_t stream);
int wfae_series_decomp_bwd(const float* dseasonal, const float* dtrend, float* dx, int B, int L, int M, int K,
                           wfae_stream_t stream);
int wfae_dlinear_frames(const float* a, const float* v, float* out, int B, int R, int M, int L, int P, int cf, int mode,
                        wfae_stream_t stream);

/* ---- intensity-statistics MLP forecaster (reference experiments/v1_experiments/prediff_mlp_sevir/train.py:20-38 `MLP`,
 * :56-70 training_step).  Added within ABI version 103; nothing changed.
 * seq_intensity_stats: seq is a batch of B sequences of T frames of HW pixels, fp32, in one of two memory orders:
 *   t_innermost = 0: (B, T, HW), every frame contiguous — what the 'NHWT' loader view has underneath;
 *   t_innermost != 0: (B, HW, T), the frame index fastest — a contiguous 'NHWT' tensor.
 *   x (B, t_in) = the mean of each of the first t_in frames.  The other P = T - t_in frames, frame-major, are cut into
 *   `groups` chunks of P HW / groups consecutive elements: target (B, 2 groups) = the chunk means, then the chunk
 *   standard deviations (unbiased, n - 1).  P % groups must be 0 (a chunk is whole frames) else WFAE_ERR_BAD_SHAPE.
 *   Every element is read once, with aligned 16-byte loads wherever a whole quad lies inside the piece a workgroup owns
 *   (seq needs 4-byte alignment only; frames need not start on a 16-byte boundary).  The first launch leaves
 *   (count, mean, M2) partials in ws — per 8192-element window of a frame (two passes over registers), or per frame and
 *   workgroup in the (B, HW, T) order (shifted sums per lane, pooled by frame) — the second pools them in fp64 in a
 *   fixed order, partials -> frames -> groups: n = sum n_k, mean = sum n_k mean_k / n, M2 = sum (M2_k + n_k (mean_k -
 *   mean)^2), the K-way form of Chan's update.  E[x^2] - E[x]^2 is never formed.  No atomics: results are bitwise
 *   repeatable.
 *   ws >= seq_intensity_stats_ws_bytes.  T <= 256.
 * mlp3_mse: pred (B, out) = W3 relu(W2 relu(W1 x + b1) + b2) + b3 for x (B, in), W1 (hidden, in), W2 (hidden, hidden),
 *   W3 (out, hidden) (nn.Linear layout); loss[0] = mean((pred - target)^2) (fp64 sum, fixed order); dw1 .. db3 = the
 *   gradients of loss with respect to the six parameters (overwritten) — all in ONE launch of one workgroup, fp32,
 *   fixed summation order.  forward_only != 0: pred only (and loss when target and loss are both given); the gradient
 *   pointers are ignored.  Served: in, out <= 32, hidden <= 256, B <= 64 (one workgroup carries the whole step), else
 *   WFAE_ERR_UNSUPPORTED.  ws >= (4 B hidden + B out) floats (2 B hidden when forward_only). */
size_t wfae_seq_intensity_stats_ws_bytes(int B, int T, int64_t HW, int t_innermost);
int wfae_seq_intensity_stats(const float* seq, float* x, float* target, int B, int T, int64_t HW, int t_in, int groups,
                             int t_innermost, void* ws, size_t ws_bytes, wfae_stream_t stream);
int wfae_mlp3_mse(const float* x, const float* target, const float* w1, const float* b1, const float* w2,
                  const float* b2, const float* w3, const float* b3, float* pred, float* loss, float* dw1, float* db1,
                  float* dw2, float* db2, float* dw3, float* db3, int B, int in, int hidden, int out, int forward_only,
                  void* ws, size_t ws_bytes, wfae_stream_t stream);

/* ---- conv latent autoencoder (reference experiments/v1_experiments/pretrained_ae_convae_sevir/train.py:58-143
 * `ConvEncoder`, `ConvDecoder`, `ConvModel`; :155 `nn.HuberLoss`).
 * The fused unit ("CLN"): y (N, Cout, Ho, Wo) = LeakyReLU_slope(LN(conv(x) + bias) * gamma + beta), x (N, Cin, H, W).
 *   kind 0: Conv2d 3x3 stride 1 pad 1 (Ho = H), w (Cout, Cin, 3, 3); kind 1: Conv2d 4x4 stride 2 pad 1 (Ho = H / 2, H and
 *   W even), w (Cout, Cin, 4, 4); kind 2: ConvTranspose2d 4x4 stride 2 pad 1 (Ho = 2 H), w (Cin, Cout, 4, 4).
 *   LN = nn.LayerNorm([Cout, Ho, Wo]): mean and biased variance per sample over E = Cout Ho Wo elements (two passes),
 *   eps 1e-5, gamma / beta (Cout, Ho, Wo) per element.  LeakyReLU: a > 0 ? a : slope * a.
 *   Served: Cin <= 64, Cout <= 16, E <= 18432 (one workgroup holds a sample's pre-norm output in LDS); anything else
 *   returns WFAE_ERR_UNSUPPORTED / WFAE_ERR_BAD_SHAPE.
 * cln_fwd writes y and, for the backward, xhat (N, Cout, Ho, Wo) = the normalised pre-affine value, mean (N), rstd (N).
 *   The pre-norm convolution output is never stored.
 * cln_bwd: from dy, xhat, rstd, gamma, beta (the mask is recomputed from a = gamma xhat + beta: a > 0 ? 1 : slope, as
 *   EW_LRELU_BWD), x and w: dx (N, Cin, H, W) (skipped when dx is null), dw, dbias (Cout), dgamma, dbeta (Cout, Ho, Wo).
 *   All outputs are overwritten.  ws >= N (|w| + Cout) floats: per-sample partials of dw and dbias, summed over the
 *   samples in ascending order by a finalize kernel, like dgamma / dbeta.  No atomics: results are bitwise repeatable.
 * huber: loss = mean of 0.5 d^2 (|d| <= delta) or delta (|d| - 0.5 delta), d = pred - target (fp64 partials, fixed-order
 *   finalize, ws >= 1024 doubles); dpred = gloss * clamp(d, -delta, delta) / n. */
int wfae_cln_fwd(const float* x, const float* w, const float* bias, const float* gamma, const float* beta, float* y,
                 float* xhat, float* mean, float* rstd, int kind, int N, int Cin, int Cout, int H, int W, float slope,
                 wfae_stream_t stream);
int wfae_cln_bwd(const float* dy, const float* xhat, const float* rstd, const float* gamma, const float* beta,
                 const float* x, const float* w, float* dx, float* dw, float* dbias, float* dgamma, float* dbeta,
                 int kind, int N, int Cin, int Cout, int H, int W, float slope, void* ws, size_t ws_bytes,
                 wfae_stream_t stream);
int wfae_huber_fwd(const float* pred, const float* target, float* loss, int64_t n, float delta, void* ws,
                   size_t ws_bytes, wfae_stream_t stream);
int wfae_huber_bwd(const float* pred, const float* target, const float* gloss, float* dpred, int64_t n, float delta,
                   wfae_stream_t stream);

/* ---- AutoencoderKL forward: the frozen latent provider, and the forward of training (backward: the block below) (reference pipeline/models/autoencoderkl/autoencoder_kl.py
 * `AutoencoderKL`; vae.py `Encoder`, `Decoder`; resnet.py `ResnetBlock2D`, `Downsample2D`, `Upsample2D`; attention.py
 * `AttentionBlock`; distributions.py `DiagonalGaussianDistribution`).  Added within ABI version 103; nothing changed.
 * conv3: 3x3 convolution, NCHW fp32, implicit GEMM on the matrix cores with fp32 accumulation.
 *   kind 0: stride 1, pad 1 (Ho = H).  kind 1: stride 2 over the input zero-padded (0, 1, 0, 1) (`Downsample2D` with
 *   padding = 0; Ho = (H - 2) / 2 + 1).  kind 2: stride 1, pad 1 over the nearest x2 upsample of x (`Upsample2D` + conv;
 *   Ho = 2 H) — the upsampled tensor is never written.
 *   mode 3: operands as three exact bf16 planes, six v_mfma_f32_16x16x32_bf16 per product (fp32-exact; 'highest' /
 *   'high').  mode 1: the h plane alone = operands rounded to bf16 ('medium').  mode 4: fp32 operands on
 *   v_mfma_f32_16x16x4_f32 (fp32-exact; kept for the comparison in DESIGN.md).
 *   The weights (Cout, Cin, 3, 3) are packed (and split) once with conv3_pack into conv3_pack_bytes bytes for a mode.
 *   Prologue (gn_scale / gn_shift (N, Cin), both or neither): the operand is SiLU(x * scale + shift) — GroupNorm folded
 *   by gn_stats — applied on the load; padding taps are zeros AFTER it.  Epilogue: y = (conv + bias (may be null) + res
 *   (y's shape, may be null)) * out_mul.  Channel counts 1..4096 (padded to 32 / 64 inside); other arguments out of range
 *   return WFAE_ERR_BAD_SHAPE / WFAE_ERR_UNSUPPORTED.
 * gn_stats: GroupNorm statistics per (sample, group), biased variance, two-level fixed-order reduction of (mean, M2)
 *   pairs in fp64 (no atomics, no E[x^2] - E[x]^2): mean, rstd (N, groups); scale = gamma rstd and
 *   shift = beta - mean rstd gamma (N, C).  ws >= gn_ws_bytes.
 * to_tokens: tok (N, S, C) = x (N, C, S) * scale + shift (scale / shift may both be null); from_tokens: y (N, C, S) =
 *   (tok (N, S, C) + res (N, C, S) (may be null)) * mul.  C and S multiples of 32.
 * softmax: y[row] = softmax(scale * x[row]) over `cols` (in place allowed).
 * posterior: moments (N, 2C, HW) -> mean, logvar = clamp(., -30, 20), std = exp(logvar / 2), and — when noise and
 *   sample are given — sample = mean + std * noise, all (N, C, HW).
 * posterior_seq (added for experiments/ae_s2, within ABI version 103; nothing changed): the sample alone for a frame
 *   sequence.  moments (B * T, 2C, HW) with frame f = b * T + t, noise (T, B, C, HW) — draw t is the noise of frame t of
 *   every sequence — -> z (B, T, C, HW), the bits of posterior's sample for the same element; mean, logvar and std are not
 *   written.  16-byte accesses when HW % 4 == 0 and the three pointers are 16-byte aligned, else scalar. */
size_t wfae_aekl_conv3_pack_bytes(int Cout, int Cin, int mode);
int wfae_aekl_conv3_pack(const float* w, void* packed, int Cout, int Cin, int mode, wfae_stream_t stream);
int wfae_aekl_conv3_fwd(const float* x, const void* packed, const float* bias, const float* gn_scale, const float* gn_shift,
                        const float* res, float* y, int kind, int mode, int N, int Cin, int Cout, int H, int W,
                        float out_mul, wfae_stream_t stream);
size_t wfae_aekl_gn_ws_bytes(int N, int C, int HW, int groups);
int wfae_aekl_gn_stats(const float* x, const float* gamma, const float* beta, float* mean, float* rstd, float* scale,
                       float* shift, int N, int C, int HW, int groups, float eps, void* ws, size_t ws_bytes,
                       wfae_stream_t stream);
int wfae_aekl_to_tokens(const float* x, const float* scale, const float* shift, float* tok, int N, int C, int S,
                        wfae_stream_t stream);
int wfae_aekl_from_tokens(const float* tok, const float* res, float* y, int N, int C, int S, float mul, wfae_stream_t stream);
int wfae_aekl_softmax(const float* x, float* y, int64_t rows, int cols, float scale, wfae_stream_t stream);
int wfae_aekl_posterior(const float* moments, const float* noise, float* mean, float* logvar, float* std_, float* sample, int N,
                        int C, int HW, wfae_stream_t stream);
int wfae_aekl_posterior_seq(const float* moments, const float* noise, float* z, int B, int T, int C, int HW,
                            wfae_stream_t stream);

/* ---- AutoencoderKL backward (csrc/aekl_bwd.hip): what `AutoencoderKL.unfreeze()` trains with.  NCHW fp32, fixed summation
 * order, no atomics: two launches give the same bits.  Added within ABI version 103; nothing changed.
 * kind, mode, N, Cin, Cout, H, W are those of the wfae_aekl_conv3_fwd call being differentiated (x (N, Cin, H, W),
 * dy (N, Cout, Ho, Wo)), with its range checks.
 * conv3_bwd_data: du (N, Cin, H, W) = conv(dy, w rotated 180 degrees, in / out transposed) * silu'(x * scale + shift),
 *   silu'(u) = s (1 + u (1 - s)), s = sigmoid(u): the gradient of the forward prologue's pre-activation.  Null gn_scale /
 *   gn_shift (both or neither): no factor, x may be null.  packed_t: w.flip(2, 3).transpose(0, 1) (Cin, Cout, 3, 3) packed
 *   with wfae_aekl_conv3_pack(wt, packed_t, Cin, Cout, mode).  kind 1 reads dy through zero insertion; kind 2 runs on the
 *   2H x 2W grid and adds up each 2 x 2 block in the epilogue (no 4x tensor).  Modes 1, 3, 4.
 * conv3_bwd_weight: dw (Cout, Cin, 3, 3) = sum over samples and output pixels of dy * a, a = SiLU(x * scale + shift)
 *   recomputed on the load (null scale / shift: a = x), padding taps zero after it; written, not accumulated.  dbias (Cout,
 *   may be null) = sum of dy.  On v_mfma_f32_16x16x32_bf16 with the pixels as K: mode 3 exact three-plane operands, mode 1
 *   operands rounded to bf16 after the prologue, mode 4 WFAE_ERR_UNSUPPORTED.  The pixel reduction is split by sample and
 *   by groups of 8 pixel tiles into slabs of ws (>= conv3_wgrad_ws_bytes, 16-byte aligned) that a finalize launch adds in
 *   ascending order.
 * gn_bwd: GroupNorm backward.  du (N, C, HW) is the gradient of u = gamma xhat + beta, xhat = (x - mean) rstd with
 *   mean / rstd (N, groups) from gn_stats.  s1 = sum du gamma_c, s2 = sum du gamma_c xhat per (sample, group),
 *   m = C / groups * HW:  dx = rstd (du gamma_c - (s1 + xhat s2) / m) + skip (dx's shape, may be null: the gradient
 *   arriving on the residual path);  dbeta[c] = sum du, dgamma[c] = sum du xhat over samples and pixels (fp64 partials,
 *   written, not accumulated).  ws >= gn_bwd_ws_bytes, 8-byte aligned; N * C <= 65535.
 * softmax_bwd: ds[row] = p (dp - sum_j p_j dp_j) scale for y = softmax(scale * x) (in place over dp allowed).
 * posterior_bwd: dmoments (N, 2C, HW) from dz (N, C, HW; may be null), the noise of the sample (null: z was the mean), the
 *   raw moments and gkl (N; may be null), the gradient of each sample's KL 0.5 sum(mean^2 + var - 1 - logvar):
 *   dmean = dz + gkl mean;  dlogvar = (0.5 dz noise std + 0.5 gkl (var - 1)) * [-30 <= raw logvar <= 20] (inclusive, as
 *   torch.clamp's gradient). */
int wfae_aekl_conv3_bwd_data(const float* dy, const void* packed_t, const float* x, const float* gn_scale, const float* gn_shift,
                             float* du, int kind, int mode, int N, int Cin, int Cout, int H, int W, wfae_stream_t stream);
size_t wfae_aekl_conv3_wgrad_ws_bytes(int kind, int N, int Cin, int Cout, int H, int W);
int wfae_aekl_conv3_bwd_weight(const float* dy, const float* x, const float* gn_scale, const float* gn_shift, float* dw,
                               float* dbias, int kind, int mode, int N, int Cin, int Cout, int H, int W, void* ws,
                               size_t ws_bytes, wfae_stream_t stream);
size_t wfae_aekl_gn_bwd_ws_bytes(int N, int C, int groups);
int wfae_aekl_gn_bwd(const float* du, const float* x, const float* gamma, const float* mean, const float* rstd, const float* skip,
                     float* dx, float* dgamma, float* dbeta, int N, int C, int HW, int groups, void* ws, size_t ws_bytes,
                     wfae_stream_t stream);
int wfae_aekl_softmax_bwd(const float* p, const float* dp, float* ds, int64_t rows, int cols, float scale, wfae_stream_t stream);
int wfae_aekl_posterior_bwd(const float* dz, const float* noise, const float* moments, const float* gkl, float* dmoments, int N,
                            int C, int HW, wfae_stream_t stream);

/* ---- LPIPS perceptual loss of the AE+GAN step (reference pipeline/models/autoencoderkl/losses/lpips.py `LPIPS`,
 * `ScalingLayer`, `vgg16`, `normalize_tensor`, `spatial_average`; used by experiments/ae_v2_2/train.py:56-60): forward and
 * the gradient with respect to the first image.  The VGG16 is frozen: no weight gradients.  NCHW fp32, fixed summation
 * order, no atomics.  Added within ABI version 103; nothing changed.
 * conv3_fwd: y (N, Cout, H, W) = max(conv3x3(x (N, Cin, H, W), stride 1, pad 1) + bias (Cout), 0).  The kernel, the modes
 *   (1 / 3 / 4) and the packed weights are those of wfae_aekl_conv3_fwd kind 0: pack (Cout, Cin, 3, 3) with
 *   wfae_aekl_conv3_pack(w, packed, Cout, Cin, mode).
 * conv3_bwd_data: dx (N, Cin, H, W) = conv3x3(dy (N, Cout, H, W), w rotated 180 degrees with in / out transposed) *
 *   (a_prev > 0); a_prev (dx's shape, may be null: no mask) is the post-ReLU activation that fed the layer, so dx is the
 *   gradient of its pre-activation.  packed_t: w.flip(2, 3).transpose(0, 1) (Cin, Cout, 3, 3) packed with
 *   wfae_aekl_conv3_pack(wt, packed_t, Cin, Cout, mode).
 *   Both: channel counts 1..4096 (else WFAE_ERR_UNSUPPORTED); N, H, W >= 1, H, W <= 8192, a sample below 2^31 elements,
 *   N * ceil(Cout / 64) <= 65535, a known mode, packed 16-byte aligned (else WFAE_ERR_BAD_SHAPE).
 * pool_fwd: y (N, C, H / 2, W / 2) = 2 x 2 stride-2 max-pool of x (N, C, H, W), floor on odd sizes; H, W >= 2.
 * pool_bwd: the gradient of the pool INPUT's pre-activation in one pass.  a (N, C, H, W) is the pool's input, a post-ReLU
 *   activation; dy (N, C, H / 2, W / 2); add (a's shape, may be null) a second gradient of a (the distance gradient of the
 *   tap):  dpre[y, x] = ((a[y, x] is the FIRST maximum of its window in the order (0,0), (0,1), (1,0), (1,1) — torch's
 *   routing) ? dy : 0) + add[y, x], times (a[y, x] > 0).  A last odd row / column belongs to no window: add only.
 * dist_fwd: one tap layer.  f = a / (sqrt(sum_c a^2) + 1e-10) for a0 and a1 (N, C, HW);
 *   out[n] += 1 / HW * sum_pixels sum_c lin[c] (f0 - f1)^2  (out (N) must be initialised; ws >= dist_ws_bytes(N, HW),
 *   8-byte aligned).  C in {64, 128, 256, 512} (else WFAE_ERR_UNSUPPORTED); N <= 65535.
 * dist_bwd: da0 (N, C, HW) = g[n] * d out[n] / d a0 (a1 has no gradient); relu != 0: times (a0 > 0), for a tap that no
 *   pool follows.  DEVIATION from the reference: at a pixel whose a0 is zero in every channel the reference's autograd
 *   gives NaN (0 * inf through the square root); here the term  - a0 / ||a0|| * (...)  is dropped there and the result
 *   is the finite  u / 1e-10.
 * prep_fwd: y (N, 3, HW) = (x (N, Cx, HW) - shift[c]) / scale[c]; Cx = 1 (every output channel reads channel 0, the
 *   reference's repeat(1, 3, 1, 1)) or 3 (else WFAE_ERR_UNSUPPORTED).  shift, scale: 3 device floats.
 * prep_bwd: dx (N, Cx, HW) = dy[c] / scale[c] (Cx = 3) or (dy[0] / scale[0] + dy[1] / scale[1]) + dy[2] / scale[2].
 * Null pointers return WFAE_ERR_NULL_POINTER, counts < 1 WFAE_ERR_BAD_SHAPE, all before any launch. */
int wfae_lpips_conv3_fwd(const float* x, const void* packed, const float* bias, float* y, int mode, int N, int Cin, int Cout,
                         int H, int W, wfae_stream_t stream);
int wfae_lpips_conv3_bwd_data(const float* dy, const void* packed_t, const float* a_prev, float* dx, int mode, int N, int Cin,
                              int Cout, int H, int W, wfae_stream_t stream);
int wfae_lpips_pool_fwd(const float* x, float* y, int N, int C, int H, int W, wfae_stream_t stream);
int wfae_lpips_pool_bwd(const float* a, const float* dy, const float* add, float* dpre, int N, int C, int H, int W,
                        wfae_stream_t stream);
size_t wfae_lpips_dist_ws_bytes(int N, int HW);
int wfae_lpips_dist_fwd(const float* a0, const float* a1, const float* lin, float* out, int N, int C, int HW, void* ws,
                        size_t ws_bytes, wfae_stream_t stream);
int wfae_lpips_dist_bwd(const float* a0, const float* a1, const float* lin, const float* g, float* da0, int N, int C, int HW,
                        int relu, wfae_stream_t stream);
int wfae_lpips_prep_fwd(const float* x, const float* shift, const float* scale, float* y, int N, int Cx, int HW,
                        wfae_stream_t stream);
int wfae_lpips_prep_bwd(const float* dy, const float* scale, float* dx, int N, int Cx, int HW, wfae_stream_t stream);

/* ---- sigmoid + L1 loss (ae_64x8x8_lin.py:102 + experiments/ae_v2/train.py:55)
 * recon = sigmoid(h); loss[0] = weight * mean |recon - x|  (fp64 accumulation).
 * bwd: dh = gloss[0] * weight * sign(recon-x) * recon*(1-recon) / n */
int wfae_sigmoid_l1_fwd(const float* h, const float* x, float* recon, float* loss, float weight,
                        int64_t n, void* ws, size_t ws_bytes, wfae_stream_t stream);
int wfae_sigmoid_l1_bwd(const float* recon, const float* x, const float* gloss, float weight,
                        float* dh, int64_t n, wfae_stream_t stream);
/* plain L1 (F.l1_loss) on an existing reconstruction: loss and dL/drecon */
int wfae_l1_fwd(const float* recon, const float* x, float* loss, float weight, int64_t n, void* ws,
                size_t ws_bytes, wfae_stream_t stream);
int wfae_l1_bwd(const float* recon, const float* x, const float* gloss, float weight, float* drecon,
                int64_t n, wfae_stream_t stream);

/* ---- SSIM / PSNR (pytorch_msssim.ssim at experiments/ae_v2/train.py:62;
 * torchmetrics SSIM/PSNR at pipeline/metrics.py:71-84).  11-tap Gaussian
 * sigma 1.5, valid window, K=(0.01,0.03), data_range 1.
 * ssim_fwd: out[0] = mean over images of mean over the (H-10)x(W-10) map.
 * ssim_bwd: dy = gout[0] * d ssim / d y  (gradient w.r.t. the second image).
 * psnr: out[0] = mean_n 10 log10(range_n^2 / mse_n), range_n = max-min of
 * target n; clamp01 != 0 clamps both inputs to [0,1] first (metrics.py:92-93). */
int wfae_ssim_fwd(const float* x, const float* y, float* out, int NB, int H, int W, int clamp01,
                  void* ws, size_t ws_bytes, wfae_stream_t stream);
int wfae_ssim_bwd(const float* x, const float* y, const float* gout, float* dy, int NB, int H, int W,
                  void* ws, size_t ws_bytes, wfae_stream_t stream);
int wfae_psnr(const float* pred, const float* target, float* out, int NB, int HW, int clamp01,
              void* ws, size_t ws_bytes, wfae_stream_t stream);

/* ---- forecast-skill scores (pipeline/metrics.py:9-68: _hit_miss_fa_cn, crps, csi, hss; calc_metrics :86-133).
 * pred (B, N, TC, H, W) — N = 1 for a deterministic (B, T, C, H, W) forecast — and target (B, TC, H, W); every
 * (b, tc) plane is one image.  `thresholds` (n_thr <= 8 floats), `pool_types` (0 none, 1 avg, 2 max) and
 * `pool_scales` (n_pools <= 3, F.*_pool2d(s, stride=s), remainder rows / columns dropped, 1 <= s <= min(H, W); the
 * scale of a `none` pool is ignored) are HOST arrays.  clamp01 != 0 clamps both inputs to [0,1] first (:92-93).
 * out (device, n_pools x (3 n_thr + 2) int64): per pool [tp, fn, fp] per threshold on the pooled ensemble mean
 * (tn = cells - tp - fn - fp), the fp64 sum over pooled cells of the CRPS expression (:36-40, eps 1e-10; mean and
 * Bessel std over the N pooled members, std 0 at N = 1) stored as the bits of a double, and the pooled cell count.
 * Pooled values are formed in torch's CPU order (sequential row-major window sum, then / s^2; sequential sum over
 * N, then / N), so the counts equal the reference's bit for bit.  ws: >= 200 bytes per partial block (<= 3 x 1024).
 * ensemble_mean: out[o][k] = sum_n pred[o][n][k] / N in that order (pred.mean(dim=1)), clamp01 as above. */
int wfae_skill_scores(const float* pred, const float* target, int64_t* out, int B, int N, int TC, int H, int W,
                      const float* thresholds, int n_thr, const int* pool_types, const int* pool_scales, int n_pools,
                      int clamp01, void* ws, size_t ws_bytes, wfae_stream_t stream);
int wfae_ensemble_mean(const float* pred, float* out, int64_t outer, int N, int64_t inner, int clamp01,
                       wfae_stream_t stream);

/* ---- forecast verification per lead time (csrc/verify.hip): wfae_verify_leads, declared in a header of its own. */
#include "wfae_verify.h"

/* ---- latent transformer of the `_tf` variant (pipeline/models/ae_64x8x8_tf.py:77-80,107-109):
 * nn.TransformerEncoderLayer(d_model=64, nhead=8, dim_feedforward=2048, dropout=0.1), post-norm, ReLU,
 * batch_first=False.  The Linear layers use wfae_linear_*.
 * layernorm: y = LN(x + res) (res may be null); mean/rstd per row are saved for backward; bwd returns the
 *   gradient w.r.t. (x + res) plus dgamma/dbeta.
 * mha_seqfirst: qkv rows are (s, n) pairs (row = s*N + n) with columns [q | k | v], E = H*D each; attention over
 *   the S axis per (n, head), softmax(q k^T / sqrt(D)), dropout on the probabilities from a counter-based
 *   generator keyed by `seed` (the same seed regenerates the mask in backward).  S <= 64, D in {8, 16}.
 * dropout: y = x * mask / (1 - p), mask from (seed, element index); applying it to dy with the same seed is
 *   the backward. */
int wfae_layernorm_fwd(const float* x, const float* res, const float* gamma, const float* beta, float* y,
                       float* mean, float* rstd, int rows, int E, float eps, wfae_stream_t stream);
int wfae_layernorm_bwd(const float* dy, const float* x, const float* res, const float* gamma, const float* mean,
                       const float* rstd, float* dx, float* dgamma, float* dbeta, int rows, int E, int accumulate,
                       void* ws, size_t ws_bytes, wfae_stream_t stream);
/* mha: the same with a layout switch — batch_first = 0: row = s*N + n (above); batch_first = 1: row = n*S + s, i.e. qkv
 * is (N batch elements, S tokens, 3E) as nn.TransformerEncoderLayer(batch_first=True) of AE_ViT_2048 has it
 * (pipeline/models/ae_vit.py:104-109).  S <= 64, D in {8, 16, 64}. */
int wfae_mha_fwd(const float* qkv, float* out, float* probs, int S, int N, int H, int D, int batch_first, float p_drop,
                 uint64_t seed, wfae_stream_t stream);
int wfae_mha_bwd(const float* qkv, const float* probs, const float* dout, float* dqkv, int S, int N, int H, int D,
                 int batch_first, float p_drop, uint64_t seed, wfae_stream_t stream);
int wfae_mha_seqfirst_fwd(const float* qkv, float* out, float* probs, int S, int N, int H, int D, float p_drop,
                          uint64_t seed, wfae_stream_t stream);
int wfae_mha_seqfirst_bwd(const float* qkv, const float* probs, const float* dout, float* dqkv, int S, int N, int H,
                          int D, float p_drop, uint64_t seed, wfae_stream_t stream);
int wfae_relu_fwd(const float* x, float* y, int64_t n, wfae_stream_t stream);
int wfae_relu_bwd(const float* dy, const float* y, float* dx, int64_t n, wfae_stream_t stream);
int wfae_dropout(const float* x, float* y, int64_t n, float p_drop, uint64_t seed, wfae_stream_t stream);

/* ---- Path-B token autoencoder AE_ViT_2048 (pipeline/models/ae_vit.py:84-162), pieces beyond the kernels above.
 * patchify / unpatchify: image (B,C,Hp*P,Wp*P) <-> rows (B*Hp*Wp, C*P*P) — the permutation that turns
 *   Conv2d(C, E, P, P) (:99) and ConvTranspose2d(E, C, P, P) (:128) into linear GEMMs; unpatchify adds bias[c].
 * add_bcast: out[o][i] = x[o][i] + p[i] (positional tokens, :142,158).
 * sq_attn: single-query attention of GlobalCrossEncode (:22-42): q (B, H*D) already projected, kv rows (b, l)
 *   with columns [k | v] (H*D each, as `.view(B, L, 2, nh, dh)` lays them out), softmax(q.k / sqrt(D)) over
 *   the L <= 64 tokens, out (B, H*D), probs (B, H, L) saved for backward. */
int wfae_patchify(const float* img, float* rows, int B, int C, int Hp, int Wp, int P, wfae_stream_t stream);
int wfae_unpatchify(const float* rows, const float* bias, float* img, int B, int C, int Hp, int Wp, int P,
                    wfae_stream_t stream);
int wfae_add_bcast(const float* x, const float* p, float* out, int64_t outer, int64_t inner, wfae_stream_t stream);
/* strided row copy: dst[r][dst_off + c] = src[(r / row_div) * src_ld + src_off + c], c < cols, r < rows; dst rows are
 * dst_ld floats long; zero_fill: the other columns of each dst row are written as 0.  The layout-only steps of
 * AE_ViT_2048.forward (pipeline/models/ae_vit.py:135 `query_vec.expand`, :86 the value slice of a fused k/v projection,
 * :89 one token copied to all positions) and their gradients. */
int wfae_copy_rows(const float* src, float* dst, int64_t rows, int cols, int64_t src_ld, int src_off, int row_div,
                   int dst_ld, int dst_off, int zero_fill, wfae_stream_t stream);
/* sum_mid: out[a][b] = sum_m x[a][m][b] (gradient of a row broadcast over the token axis) */
int wfae_sum_mid(const float* x, float* out, int64_t A, int M, int64_t Bn, wfae_stream_t stream);
int wfae_sq_attn_fwd(const float* q, const float* kv, float* out, float* probs, int B, int L, int H, int D,
                     wfae_stream_t stream);
int wfae_sq_attn_bwd(const float* q, const float* kv, const float* probs, const float* dout, float* dq, float* dkv, int B,
                     int L, int H, int D, wfae_stream_t stream);

/* ---- AdamW (torch.optim.AdamW via pipeline/helpers.py:63-74) ---------------
 * p *= 1 - lr*wd;  m = b1 m + (1-b1) g;  v = b2 v + (1-b2) g^2;
 * p -= lr/bc1 * m / (sqrt(v)/sqrt(bc2) + eps),  g pre-multiplied by grad_scale
 * (1/world_size after a sum all-reduce). */
int wfae_adamw(float* p, const float* g, float* m, float* v, int64_t n, float lr, float beta1,
               float beta2, float eps, float weight_decay, float bias_corr1, float bias_corr2,
               float grad_scale, wfae_stream_t stream);
/* The same with the complements 1 - beta1 and 1 - beta2 passed in: torch forms them from the Python doubles and rounds
 * once, while 1.f - 0.999f is 1.3e-5 short of 0.001, which scales every step by 1 + 6.4e-6 (visible on parameters that
 * start at zero, such as biases).  wfae_adamw keeps forming them in fp32 from the rounded betas and is what
 * FusedAdamW calls unless it is built with exact_complements=True. */
int wfae_adamw_c(float* p, const float* g, float* m, float* v, int64_t n, float lr, float beta1, float beta2,
                 float one_minus_beta1, float one_minus_beta2, float eps, float weight_decay, float bias_corr1,
                 float bias_corr2, float grad_scale, wfae_stream_t stream);
/* out[0] = sum x^2 (fp64 accumulation, written as fp64): grad-norm tracking
 * (pipeline/helpers.py:250-256) */
int wfae_sumsq(const float* x, int64_t n, double* out, void* ws, size_t ws_bytes,
               wfae_stream_t stream);

/* ---- loader contract on device (pipeline/datasets/sevire/sevir.py:749-794,
 * 98-139): uint8 VIL (NB,H,W,T) 'NHWT' -> fp32 (NB,T,H,W) 'NTHW' scaled by
 * 1/255. */
int wfae_vil_u8_to_f32(const uint8_t* src, float* dst, int NB, int H, int W, int T, float scale,
                       wfae_stream_t stream);
/* The same conversion with the train-time augmentation of the reference's second loader fused in
 * (pipeline/datasets/sevir/sevir.py:1035-1058: h-flip, v-flip, then torchvision's rotate with its defaults: nearest
 * neighbour, no expand, centre of the image, zero fill), one transform per sample applied to all T frames.
 * xf is a device fp32 (NB,4): cos(theta), sin(theta), hflip (0/1), vflip (0/1); theta counter-clockwise.  For output
 * pixel (i, j), in fp32:
 *   x_o = j + 0.5 - W/2,  y_o = i + 0.5 - H/2
 *   xs = rintf(cos * x_o - sin * y_o + W/2 - 0.5),  ys = rintf(sin * x_o + cos * y_o + H/2 - 0.5)   (half to even)
 *   dst[n][t][i][j] = scale * (0.f + 0.f)                                          if (ys, xs) is outside the image
 *                   = scale * ((float)src[n][vflip ? H-1-ys : ys][hflip ? W-1-xs : xs][t] + 0.f)     otherwise
 * The bounds test is made on the rounded integers, before the flips.  With the row (1, 0, 0, 0) the result is
 * bit-identical to wfae_vil_u8_to_f32; with cos, sin in {0, +1, -1} on square frames it is torch.rot90.  Any H, W, T
 * (16-byte stores where W % 4 == 0, dword stores otherwise). */
int wfae_vil_augment_u8_to_f32(const uint8_t* src, const float* xf, float* dst, int NB, int H, int W, int T, float scale,
                               wfae_stream_t stream);

/* The same conversion with a frame stride and block pooling fused in: what turns raw SEVIR (384 x 384 x 49) into
 * sevir_lr (128 x 128 x 25) at factors (2, 3, 3).  src uint8 (NB,H,W,T) 'NHWT'; dst fp32 (NB,To,Ho,Wo) 'NTHW' with
 * To = ceil(T / ft); output frame t' is raw frame t' * ft.
 *   mode 0 (max): the reference's offline recipe (pipeline/datasets/sevire/sevir.py:575-616, [..., ::ft] then
 *     block_reduce(block_size=(1, fh, fw, 1), func=np.max)).  Ho = ceil(H / fh), Wo = ceil(W / fw); a block that sticks
 *     out of the image is reduced over its pixels inside (block_reduce pads with 0: the same for a max over uint8).
 *   mode 1 (mean): the reference's runtime downsample_data_dict (:849-890, [::ft] then avg_pool2d(kernel_size=(fh, fw))).
 *     Ho = H / fh, Wo = W / fw (floor): the remainder is dropped, as avg_pool2d drops it.
 * Arithmetic, fp32, every operation rounded on its own (no fma, no reciprocal):
 *   v(b)  = scale * ((float)b + offset)                        one add, then one multiply
 *   max:  out = v(max of the block's bytes)
 *   mean: acc = 0.f; for a in [0, fh): for b in [0, fw): acc = acc + v(byte[a][b]);  out = acc / (float)(fh * fw)
 *     (bit-identical to torch.nn.functional.avg_pool2d of scale * (u8.float() + offset) on the CPU)
 * Geometry: xf == NULL: output pixel (i, j) reduces block (i, j).  Otherwise xf is the device fp32 (NB,4) of
 * wfae_vil_augment_u8_to_f32, applied on the POOLED grid Ho x Wo: the source pixel of its formula names the block to
 * reduce, and a pixel whose rotated centre falls outside is exactly 0.f, whatever the offset (the reference rotates after
 * preprocessing and fills with 0).  With ft = fh = fw = 1 and offset = 0 both modes are bit-identical to
 * wfae_vil_u8_to_f32 (xf == NULL) and to wfae_vil_augment_u8_to_f32 (with rows).
 * Errors, all before any launch: null src / dst; NB, H, W, T, ft, fh or fw < 1, H * W > INT_MAX, or mean with fh > H or
 * fw > W (WFAE_ERR_BAD_SHAPE); mode not 0 or 1 (WFAE_ERR_UNSUPPORTED).  Any alignment of src and dst rows. */
int wfae_vil_pool_u8_to_f32(const uint8_t* src, const float* xf /* may be NULL */, float* dst, int NB, int H, int W, int T,
                            int ft, int fh, int fw, int mode, float scale, float offset, wfae_stream_t stream);

/* ---- 3x3 stride-2 padding-1 convolution family of the conv + GAN latent model (csrc/c3s2.hip; reference
 * experiments/v1_experiments/pretrained_ae_conv_disc/train.py:140-188 `Encoder`, `Decoder`).  Added within ABI version
 * 103; nothing changed.
 * One weight layout w (Clo, Chi, 3, 3): Conv2d(Chi -> Clo).weight, and ConvTranspose2d(Clo -> Chi).weight.  "hi" is the
 * larger plane (N, Chi, Hhi, Whi), "lo" the smaller (N, Clo, Hlo, Wlo); Hlo = (Hhi - 1) / 2 + 1 (so Hhi = 2 Hlo - 1 +
 * output_padding, output_padding 0 or 1), likewise W.  transposed = 0: the module is Conv2d (x is hi, y is lo, bias Clo);
 * transposed = 1: ConvTranspose2d (x is lo, y is hi, bias Chi).  act: 0 = none, 1 = SiLU.
 *   wfae_c3s2_fwd:        t = conv(x) + bias (bias may be NULL), y = act(t); t may be NULL (nothing saved).
 *   wfae_c3s2_bwd_data:   dx = conv_data_gradient(da act'(t)); t is read only when act = 1.
 *   wfae_c3s2_bwd_weight: dw (and dbias unless NULL) of dt = da act'(t) against the module input x, the bias gradient from
 *                         extra workgroups of the same launch; accumulate: add to dw / dbias instead of overwriting.
 * dt is formed inside the kernels that read da.  Tap (ky, kx) is DEAD when no lo position reads a real hi pixel through it
 * (wfae_c3s2_live_taps: bit ky * 3 + kx set = live; at 2x2 -> 1x1 only ky, kx in {1, 2} are live): dead weights never enter
 * the arithmetic, dead gradients are written as exact zeros, or left untouched when accumulating.  Dead weights ARE fetched:
 * the nine taps of a (cl, ch) pair are 36 contiguous bytes, so they share their 16-byte accesses and 128-byte lines with
 * live ones and are zeroed in registers; skipping them saves arithmetic, not memory traffic.
 * Reductions are split over workgroups and finished from the workspace in a fixed order: no atomics, bitwise repeatable.
 * ws: wfae_c3s2_workspace_bytes(op, ...) bytes, op 0 = fwd, 1 = bwd_data, 2 = bwd_weight (0 for shapes that are refused).
 * Errors, all before any launch: null pointers WFAE_ERR_NULL_POINTER; a size < 1, an unknown act or a tensor of 2^31
 * elements WFAE_ERR_BAD_SHAPE; Hlo / Hhi (Wlo / Whi) that do not belong together, or more than 65535 tiles of 8 lo rows
 * (N Hlo Wlo > 524280: one grid dimension counts them), WFAE_ERR_UNSUPPORTED; a short workspace WFAE_ERR_WORKSPACE. */
int wfae_c3s2_live_taps(int Hhi, int Whi, int Hlo, int Wlo);
size_t wfae_c3s2_workspace_bytes(int op, int transposed, int N, int Chi, int Clo, int Hhi, int Whi, int Hlo, int Wlo);
int wfae_c3s2_fwd(const float* x, const float* w, const float* bias /* may be NULL */, float* y, float* t /* may be NULL */,
                  int transposed, int act, int N, int Chi, int Clo, int Hhi, int Whi, int Hlo, int Wlo, void* ws,
                  size_t ws_bytes, wfae_stream_t stream);
int wfae_c3s2_bwd_data(const float* da, const float* t, const float* w, float* dx, int transposed, int act, int N, int Chi,
                       int Clo, int Hhi, int Whi, int Hlo, int Wlo, void* ws, size_t ws_bytes, wfae_stream_t stream);
int wfae_c3s2_bwd_weight(const float* da, const float* t, const float* x, float* dw, float* dbias /* may be NULL */,
                         int transposed, int act, int accumulate, int N, int Chi, int Clo, int Hhi, int Whi, int Hlo, int Wlo,
                         void* ws, size_t ws_bytes, wfae_stream_t stream);

/* ---- conv + attention latent autoencoder (csrc/convattn.hip; reference
 * experiments/v1_experiments/pretrained_ae_convattn_ae_sevir/train.py:58-161 `ConvAttnModel`).  Added within ABI version
 * 103; nothing changed: wfae_mha_* (S <= 64) and wfae_sq_attn_* (L <= 64) above keep their kernels and their bits.
 *
 * attn: multi-head attention with separate query and key / value lengths, 1 <= Sq, Skv <= WFAE_ATTN_MAX_S, D = 16 (other
 *   head sizes: WFAE_ERR_UNSUPPORTED), any H; E = H * D.  Batch-first rows: query row n * Sq + i, key / value row
 *   n * Skv + j.  q, k, v are pointers to column 0 of their first row plus a ROW STRIDE in floats (>= E), so one pair of
 *   kernels serves a packed [q | k | v] projection (q = p, k = p + E, v = p + 2E, strides 3E, as wfae_mha_fwd takes it) and
 *   a separate q with a packed [k | v] (k = kv, v = kv + E, strides 2E, as wfae_sq_attn_fwd takes it).  out (N * Sq, E)
 *   contiguous.  P = softmax(q . k / sqrt(D)) with the row maximum subtracted; probs (N, H, Sq, Skv) holds P BEFORE
 *   dropout; dropout on P from the counter-based generator of wfae_dropout / wfae_mha_fwd with mask index
 *   ((n H + h) Sq + i) Skv + j (for Sq = Skv: wfae_mha_fwd's batch-first indexing).  bwd writes dq, dk, dv through the
 *   strides of q, k, v (the gradient of a packed projection lands in one buffer); dout (N * Sq, E) contiguous.  No
 *   atomics, fixed summation order: bitwise repeatable.  With Skv = 1: P == 1, dq == dk == 0 exactly.
 * gn_act: GroupNorm(G, C) + optional exact GELU in training form.  x (N, C, HW); bias (C) may be NULL and is added to x
 *   before the statistics (the bias of the convolution in front at no launch); y = act((x + bias - mean) rstd gamma +
 *   beta), act 0 = none, 1 = GELU (erf form); mean, rstd (N, G) saved; statistics two-pass in fp64 on the group held on
 *   chip, biased variance, rstd = 1 / sqrt(var + eps).  One launch.  bwd: dx, dgamma, dbeta and — exactly when bias was
 *   given — dbias = sum over (n, hw) of dx, from dy, x, bias and the two statistics (the activation is recomputed);
 *   accumulate: add to dgamma / dbeta / dbias.  Per-channel sums over N are finished from ws (wfae_gn_act_bwd_workspace_bytes)
 *   in a fixed order.  Errors before any launch: C % G != 0 WFAE_ERR_BAD_SHAPE; a group of more than WFAE_GN_MAX_GROUP
 *   elements (C / G * HW; 16 x 576 = 9216 is inside) WFAE_ERR_UNSUPPORTED; a short workspace WFAE_ERR_WORKSPACE.
 *   LDS per workgroup: 4 bytes per group element forward, 8 backward (128 KiB at the limit); WFAE_ERR_LAUNCH if the device
 *   does not grant it.
 * channel_bias: y[n][c][p] = x[n][c][p] + b[c] (the gradient of b is wfae_reduce_sum).
 * head_dropout_bcast: attention over ONE key in training: out[n][i][h D + d] = v[n][h D + d] keep(n, h, i) / (1 - p), mask
 *   index (n H + h) Sq + i — wfae_attn_fwd's at Skv = 1; bwd: dv[n][e] = sum_i dout[n][i][e] keep / (1 - p), i in order. */
#define WFAE_ATTN_MAX_S 256
#define WFAE_GN_MAX_GROUP 16384
int wfae_attn_fwd(const float* q, const float* k, const float* v, float* out, float* probs, int N, int Sq, int Skv, int H,
                  int D, int64_t q_stride, int64_t k_stride, int64_t v_stride, float p_drop, uint64_t seed,
                  wfae_stream_t stream);
int wfae_attn_bwd(const float* q, const float* k, const float* v, const float* probs, const float* dout, float* dq, float* dk,
                  float* dv, int N, int Sq, int Skv, int H, int D, int64_t q_stride, int64_t k_stride, int64_t v_stride,
                  float p_drop, uint64_t seed, wfae_stream_t stream);
size_t wfae_gn_act_bwd_workspace_bytes(int N, int C);
int wfae_gn_act_fwd(const float* x, const float* bias /* may be NULL */, const float* gamma, const float* beta, float* y,
                    float* mean, float* rstd, int N, int C, int HW, int G, float eps, int act, wfae_stream_t stream);
int wfae_gn_act_bwd(const float* dy, const float* x, const float* bias /* may be NULL */, const float* gamma,
                    const float* beta, const float* mean, const float* rstd, float* dx, float* dgamma, float* dbeta,
                    float* dbias /* NULL iff bias is */, int N, int C, int HW, int G, int act, int accumulate, void* ws,
                    size_t ws_bytes, wfae_stream_t stream);
int wfae_channel_bias_fwd(const float* x, const float* b, float* y, int N, int C, int HW, wfae_stream_t stream);
int wfae_head_dropout_bcast_fwd(const float* v, float* out, int N, int Sq, int H, int D, float p_drop, uint64_t seed,
                                wfae_stream_t stream);
int wfae_head_dropout_bcast_bwd(const float* dout, float* dv, int N, int Sq, int H, int D, float p_drop, uint64_t seed,
                                wfae_stream_t stream);

/* ---- residual autoencoders of ae_gan, evaluation forward (csrc/resae.hip; reference
 * experiments/v1_experiments/ae_gan/train.py:46-217 `ResidualBlock`, `UpsampleBlock`, `ConvAutoencoder`,
 * `ConvAutoencoderBIG`).  Added within ABI version 103; nothing changed.
 * resae_conv:  y = act( conv(x, w) * scale[co] + shift[co] + res ),  NCHW fp32, fp32 accumulation.
 *   kind 0: 3x3 stride 1 pad 1.  1: 3x3 stride 2 pad 1, Ho = (H - 1) / 2 + 1, input row 2 oy - 1 + ky (NOT
 *   wfae_aekl_conv3_fwd's kind 1, which pads (0, 1, 0, 1)).  2: 3x3 stride 1 pad 1 over the x2 nearest upsample of x, which
 *   is never written (Ho = 2 H).  3 / 4: 1x1 with stride 1 / 2 (w is (Cout, Cin, 1, 1)): the centre tap of kind 0 / 1.
 *   scale, shift (Cout): BatchNorm's running statistics folded per channel, scale = gamma / sqrt(running_var + eps), shift =
 *   beta - running_mean scale; either may be NULL, a plain bias is shift alone.  res_mode 0: none (res NULL); 1: res (N,
 *   Cout, Ho, Wo); 2: res (N, Cout, Ho / 2, Wo / 2) read as res[n, co, oy >> 1, ox >> 1] (Ho, Wo even).  act 0: none, 1:
 *   the exact (erf) GELU.
 *   route 0, "tile": an implicit GEMM on the matrix cores for any shape, 64 output channels x 8 x 16 pixels of one sample per
 *   workgroup; mode 1 / 3 / 4 = bf16 operands / three bf16 planes (fp32 accuracy) / fp32 MFMA, as wfae_aekl_conv3_fwd.
 *   route 1, "small": output planes of at most 16 pixels (else WFAE_ERR_UNSUPPORTED).  The GEMM's columns are the output
 *   pixels of all samples; a workgroup owns 64 output channels x 64 columns x a share of K and reads its fp32 weights once
 *   (mode is ignored: fp32 MFMA); K is split over workgroups where the output channels do not fill the chip and finished
 *   from ws (wfae_resae_workspace_bytes, 0 when no split is made) in ascending order.  A tap is DEAD when no output position
 *   of the layer reads a real input pixel through it (wfae_resae_live_taps: bit ky * 3 + kx set = live, the layout of
 *   wfae_c3s2_live_taps; kinds 3 / 4: the centre bit): dead taps are neither fetched nor multiplied, live taps that are
 *   padding for one column contribute literal zeros.
 *   Fixed summation order on both routes, no atomics: two launches give the same bits.
 * resae_pack: w (Cout, Cin, 3, 3) (kinds 0..2) or (Cout, Cin, 1, 1) (kinds 3, 4), the RAW weights, -> the operand of
 *   resae_conv for (route, kind, mode), wfae_resae_pack_bytes bytes (0 for arguments that are refused), 16-byte aligned.
 *   route 0: [plane][32-channel chunk][tap][co padded to 64][32 ci], wfae_aekl_conv3_pack's layout; route 1: fp32 in MFMA
 *   fragment order, [tap][16 co][16 ci] blocks.
 * Errors, all before any launch: null x / packed / y / w WFAE_ERR_NULL_POINTER; an unknown route, kind, mode (route 0),
 *   res_mode or act, res_mode that does not go with res, a size < 1, a plane above 8192, an odd output plane with res_mode 2,
 *   a sample of 2^31 elements, a misaligned packed WFAE_ERR_BAD_SHAPE; channel counts above 4096, and on route 1 a larger
 *   output plane or N Ho Wo >= 2^21, WFAE_ERR_UNSUPPORTED; a short or misaligned workspace WFAE_ERR_WORKSPACE. */
int wfae_resae_live_taps(int kind, int H, int W);
size_t wfae_resae_pack_bytes(int route, int kind, int mode, int Cout, int Cin);
int wfae_resae_pack(const float* w, void* packed, int route, int kind, int mode, int Cout, int Cin, wfae_stream_t stream);
size_t wfae_resae_workspace_bytes(int kind, int N, int Cin, int Cout, int H, int W);
int wfae_resae_conv(const float* x, const void* packed, const float* scale /* may be NULL */, const float* shift /* may be NULL */,
                    const float* res /* NULL iff res_mode = 0 */, float* y, int route, int kind, int mode, int res_mode, int act,
                    int N, int Cin, int Cout, int H, int W, void* ws /* may be NULL when no bytes are needed */, size_t ws_bytes,
                    wfae_stream_t stream);

/* ---- residual autoencoders of ae_gan, backward (csrc/resae_bwd.hip).  Added within ABI version 103; nothing changed.
 * kind, N, Cin, Cout, H, W are the FORWARD layer's (wfae_resae_conv): x (N, Cin, H, W), dy (N, Cout, Ho, Wo), the raw
 * weight (Cout, Cin, k, k).  NCHW fp32, the fp32 matrix instruction, fixed summation order, no atomics: two launches
 * give the same bits.  Both gradients are GEMMs over groups of 64 COLUMNS, one per pixel:
 *   route 1, "small": the columns are the pixels of all samples in (n, y, x) order; Ho Wo <= 16 and N H W < 2^21 (else
 *   WFAE_ERR_UNSUPPORTED).  route 0, "tile": a group is an 8 x 8 tile of one sample; any shape.
 *   Dead taps (wfae_resae_live_taps) are never read: their weight gradient is exactly 0.0 and their weights, whatever they
 *   hold, do not reach dx.
 * resae_bwd_pack: the raw weight -> packed_t, the data gradient's operand on both routes (in and out channels transposed,
 *   fp32 in MFMA fragment order, [tap][16 ci][16 co] blocks; the tap keeps its forward index and the kernel runs the
 *   geometry backwards, which is the 180-degree rotation), wfae_resae_bwd_pack_bytes bytes, 16-byte aligned.
 * resae_bwd_data: dx (N, Cin, H, W) = dgrad(dy) + add; add (dx's shape) may be NULL.  Written, not accumulated.  Kind 1:
 *   dy row (iy + 1 - ky) / 2 where that is exact and in range; kind 4: the 1x1 product at even positions, exact zeros
 *   elsewhere; kind 2: the gradient on the x2 grid with each 2 x 2 block summed, the upsampled tensor is never written.
 *   Where K = Cout is split over workgroups (small route), and for kind 2 on the small route, the partial sums go to ws
 *   (wfae_resae_bwd_data_workspace_bytes) and a finishing launch adds them in ascending order.
 * resae_bwd_weight: dw in the raw shape (Cout, Cin, k, k), written, not accumulated, each (co, ci)'s taps as one run;
 *   dbias (Cout) = the sum of dy over (n, oy, ox), may be NULL.  K is the columns of all samples together; where they are
 *   split over workgroups the partial dw go to ws (wfae_resae_bwd_weight_workspace_bytes; one slab per SPLIT, never per
 *   sample) and are added in ascending order.
 * resae_join_fwd: the end of a train-mode block,  y = gelu(c2 s2[c] + h2[c] + r'),  r' = r ss[c] + hs[c] (the shortcut
 *   convolution under its own BatchNorm) or r itself where ss and hs are NULL (identity shortcut); c2, y (N, C, H, W);
 *   res_mode 1: r (N, C, H, W); 2: r (N, C, H / 2, W / 2) read as r[n, c, oy >> 1, ox >> 1] (H, W even).
 * resae_join_bwd: one pass that rebuilds the pre-activation and writes dpre = dy gelu'(pre); at res_mode 2 also dres (r's
 *   shape), each 2 x 2 block of dpre summed in row-major order (dres NULL exactly at res_mode 1, where it is dpre).
 * resae_bn_running: the running-statistics update of a train-mode BatchNorm whose input is read through the x2 upsample
 *   (the shortcut of an UpsampleBlock, which runs at the source resolution): from the saved batch mean and invstd of the
 *   source tensor (wfae_bn_stats_train with NULL running statistics), with the unbiased factor count / (count - 1) for
 *   count = 4 N H W, the number of values nn.BatchNorm2d sees on the upsampled tensor.
 * Errors, all before any launch: null required pointers WFAE_ERR_NULL_POINTER; an unknown route, kind or res_mode, a size
 *   < 1, a plane above 8192, an odd plane with res_mode 2, one of ss / hs without the other, dres that does not go with
 *   res_mode, a sample of 2^31 elements, a misaligned packed_t WFAE_ERR_BAD_SHAPE; channel counts above 4096, and on route
 *   1 a larger plane, WFAE_ERR_UNSUPPORTED; a short or misaligned workspace WFAE_ERR_WORKSPACE. */
size_t wfae_resae_bwd_pack_bytes(int kind, int Cout, int Cin);
int wfae_resae_bwd_pack(const float* w, void* packed_t, int kind, int Cout, int Cin, wfae_stream_t stream);
size_t wfae_resae_bwd_data_workspace_bytes(int route, int kind, int N, int Cin, int Cout, int H, int W);
int wfae_resae_bwd_data(const float* dy, const void* packed_t, const float* add /* may be NULL */, float* dx, int route, int kind,
                        int N, int Cin, int Cout, int H, int W, void* ws /* may be NULL when no bytes are needed */,
                        size_t ws_bytes, wfae_stream_t stream);
size_t wfae_resae_bwd_weight_workspace_bytes(int route, int kind, int N, int Cin, int Cout, int H, int W);
int wfae_resae_bwd_weight(const float* dy, const float* x, float* dw, float* dbias /* may be NULL */, int route, int kind, int N,
                          int Cin, int Cout, int H, int W, void* ws /* may be NULL when no bytes are needed */, size_t ws_bytes,
                          wfae_stream_t stream);
int wfae_resae_join_fwd(const float* c2, const float* s2, const float* h2, const float* r, const float* ss /* may be NULL */,
                        const float* hs /* NULL iff ss is */, float* y, int res_mode, int N, int C, int H, int W,
                        wfae_stream_t stream);
int wfae_resae_join_bwd(const float* dy, const float* c2, const float* s2, const float* h2, const float* r,
                        const float* ss /* may be NULL */, const float* hs /* NULL iff ss is */, float* dpre,
                        float* dres /* NULL iff res_mode = 1 */, int res_mode, int N, int C, int H, int W, wfae_stream_t stream);
int wfae_resae_bn_running(const float* save_mean, const float* save_invstd, float* running_mean, float* running_var, int C,
                          float eps, float momentum, int64_t count, wfae_stream_t stream);

/* ---- prediction / target / difference panels in the SEVIR VIL colours (csrc/panels.hip; reference
 * pipeline/helpers.py:155-225 `log_wandb_images`).  Added within ABI version 103; nothing changed.
 * panel_render: pred, target fp32 (B, T, H, W) contiguous; lut_vil, lut_diff: 256 x 3 device bytes (RGB), the colours of
 *   the frame rows and of the difference row: the kernel holds no colour constants.  The first nb <= B samples are drawn,
 *   samples >= nb are never read.  out: nb figures of wfae_panel_bytes(T, H, W, g) bytes each, one after the other.
 *   A figure is Hfig = 3 H + 2 g rows of Wfig = T W + (T - 1) g pixels: row block 0 the target, 1 the prediction, 2 the
 *   difference, each T panels of H x W in frame order; g white pixels (255, 255, 255) between neighbouring panels and
 *   between row blocks.  It is written as the stream a PNG IDAT chunk holds before compression: Hfig scanlines, each a
 *   filter byte 0 followed by 3 Wfig RGB bytes, so a figure is Hfig (1 + 3 Wfig) bytes.
 *   Per pixel:  u(x) = (uint8)(min(max(x, 0), 1) * 255.0f), one fp32 multiply and a truncation toward zero, which is
 *   (x.clamp(0, 1) * 255).numpy().astype('uint8'); u(NaN) = 0 (the reference's cast is unspecified there), u(-inf) = 0,
 *   u(+inf) = 255.  d = |u(target) - u(pred)|.  Colours lut_vil[u(target)], lut_vil[u(pred)], lut_diff[d].
 * panel_bytes: the bytes of one figure; 0 for arguments that panel_render refuses.
 * range_count: *count (a device int64) = the number of the n elements of x with 0 <= x <= 1; NaN and +-inf are outside.
 *   Integer partial counts in ws (wfae_range_count_workspace_bytes(n) bytes, 8-byte aligned), added by a second launch:
 *   exact, so two launches give the same integer.
 * Errors, all before any launch: null pointers WFAE_ERR_NULL_POINTER; a size < 1, nb < 1 or nb > B, g < 0, a figure of
 *   2^31 bytes or more, n < 1 WFAE_ERR_BAD_SHAPE; a short or misaligned workspace WFAE_ERR_WORKSPACE. */
size_t wfae_panel_bytes(int T, int H, int W, int g);
int wfae_panel_render(const float* pred, const float* target, const uint8_t* lut_vil, const uint8_t* lut_diff, uint8_t* out,
                      int B, int nb, int T, int H, int W, int g, wfae_stream_t stream);
size_t wfae_range_count_workspace_bytes(int64_t n);
int wfae_range_count(const float* x, int64_t n, int64_t* count, void* ws, size_t ws_bytes, wfae_stream_t stream);

/* ---- latent cache of the frozen AutoencoderKL provider (csrc/latent_cache.hip; experiments/v1_experiments/_latents.py
 * `LatentCache`).  Added within ABI version 103; nothing changed.
 * A row is one frame's payload of L fp32 values: the posterior mode (L = C h w) or the moments (L = 2 C h w).  table:
 * (capacity, L).  slots and index are device int32.
 * latent_scatter: for m < M with 0 <= slots[m] < capacity, table[slots[m], :] = src[m, :]; slots[m] == -1 skips row m and
 *   leaves the table untouched.  Distinct rows never share a slot (the caller's contract: the rows are written without
 *   atomics).  Any other slot value is the caller's error, to be checked on the host copy the slots were built from; the
 *   kernel skips such a row rather than follow it.
 * latent_gather: output frame f = b * T + t reads row table[index[f]] if index[f] >= 0, else fresh[-1 - index[f]]
 *   (fresh: (M, L), the rows encoded this step; may be NULL with M = 0 when no index is negative).
 *   mode 0: out (B * T, L), out[f, :] = row.
 *   mode 1: the row holds moments, L = 2 CHW, noise (T, B, CHW) draw-major, out (B * T, CHW):
 *     out[f, r] = fmaf(expf(0.5f * clamp(row[CHW + r], -30, 20)), noise[(t * B + b) * CHW + r], row[r]),
 *     the expression and operand order of wfae_aekl_posterior_seq: its bits for the same moments.
 *   An index outside [-M, capacity) is the caller's error (host copy, as above); the kernel leaves such a frame unwritten.
 * Both: grid-stride streaming copies, 16-byte accesses when L % 4 == 0 (mode 1: CHW % 4 == 0) and every pointer is 16-byte
 *   aligned, scalar otherwise.  No atomics: two launches give the same bits.
 * Errors, all before any launch: null pointers (noise in mode 1; fresh with M > 0) and noise given in mode 0
 *   WFAE_ERR_NULL_POINTER; a size < 1, M < 0 (gather), a mode other than 0 or 1, mode 1 with odd L, or an array of 2^39
 *   elements WFAE_ERR_BAD_SHAPE. */
int wfae_latent_scatter(const float* src, const int* slots, float* table, int M, int L, int capacity, wfae_stream_t stream);
int wfae_latent_gather(const float* table, const float* fresh, const int* index, const float* noise, float* out, int B, int T,
                       int L, int mode, int capacity, int M, wfae_stream_t stream);

/* ---- row-invariant nn.Linear forward (csrc/linear_rowinv.hip): the attention projections of the frozen AutoencoderKL in
 * pass-invariant mode (`AutoencoderKL.pass_invariant()`, functional.aekl_attention(row_invariant=True)), and its 1x1
 * convolutions on tokens (functional.aekl_conv1x1_rowinv).  Added within ABI
 * version 103; nothing changed: 230 entry points.
 * y[b,o] = sum_i x[b,i] w[o,i] + bias[o], x (B, In), w (Out, In), bias (Out) or NULL, y (B, Out), fp32, no workspace.
 * Contract: the bits of y[b,o] are a function of x[b,:], w[o,:], bias[o], In, Out and the matmul precision only — not of B,
 *   of the row's index, of which other rows are in the call, nor of whether the pointers allow 16-byte loads.  (wfae_linear_fwd
 *   chooses its row tile, its K-split — the summation order — and at fp32 precision its instruction from B and from the
 *   workspace size.)  The tile (64 x 64 x 16) and the k-loop follow from (In, Out) alone, K is never split across
 *   workgroups, every output element is one accumulator chain over ascending k with the bias added last, rows and columns
 *   past the edge are masked.  WFAE_PRECISION_FP32: v_mfma_f32_32x32x2_f32, a k-ordered fp32 fmaf chain, whatever
 *   wfae_set_split_gemm says; WFAE_PRECISION_BF16: operands rounded to bf16 (nearest even), v_mfma_f32_32x32x16_bf16,
 *   fp32 accumulation.
 * Served: B >= 1; In and Out multiples of 32 up to 4096.
 * Errors, all before any launch: x, w or y NULL WFAE_ERR_NULL_POINTER; a size < 1 WFAE_ERR_BAD_SHAPE; any other In or Out
 *   WFAE_ERR_UNSUPPORTED. */
int wfae_linear_fwd_rowinv(const float* x, const float* w, const float* bias, float* y, int B, int In, int Out,
                           wfae_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* WFAE_H */
