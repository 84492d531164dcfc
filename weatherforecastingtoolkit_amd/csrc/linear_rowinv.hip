// linear_rowinv.hip — nn.Linear forward whose result for a row does not depend on the other rows of the call:
// y[b,o] = sum_i x[b,i] w[o,i] + bias[o], the bits of y[b,o] a function of x[b,:], w[o,:], bias[o], In, Out and the
// matmul precision alone.  It is what the frozen AutoencoderKL's attention projections run on in pass-invariant mode
// (functional.aekl_attention(row_invariant=True)) and its 1x1 convolutions on tokens (functional.aekl_conv1x1_rowinv), so
// that a frame's latent is the same bits in every encoder pass.
//
// What wfae_linear_fwd (gemm.hip) chooses from the row count — the row-tile height, the K-split and with it the
// summation order, and at fp32 precision even the instruction (the three-plane split from 64 rows on, the fp32 MFMA
// below) — is fixed here:
//   * one tile shape, 64 rows x 64 columns x 16 k, 256 threads = 2 x 2 waves of one 32 x 32 MFMA tile each;
//   * K is never split: a workgroup walks k = 0 .. In in steps of 16, every output element is ONE accumulator chain over
//     ascending k (fp32: v_mfma_f32_32x32x2_f32, bit for bit a k-ordered fmaf chain; bf16: operands rounded to nearest
//     even after the LDS read, one v_mfma_f32_32x32x16_bf16 per step, fp32 accumulation), and the bias is added last;
//   * rows >= B and columns >= Out of an edge tile are loaded as zeros from a clamped address and never stored — a row
//     of an MFMA tile depends on its own operand row only, so what shares a tile with a row does not reach its result;
//   * operands that are not 16-byte aligned are read with four scalar loads instead of one dwordx4: the same values
//     reach the same LDS words.
// The tile: one frame of the provider is 64 .. 2304 token rows and the projections are 512 wide, so a 64-row tile is
// filled by the smallest frame (a 128-row tile would be half masked) and gives 8 .. 288 workgroups for one frame,
// 3328 for a whole ae_s2 pass of 26 624 rows; 17 KiB of LDS and 16 accumulator registers leave room for 8 workgroups
// per CU, which is what hides the global-load latency of the 32-stage k-loop when only a few tiles exist.  With one MFMA
// tile per wave the fp32 instruction (64 cycles) covers its two ds_read_b32; the bf16 form is LDS-bound (16 reads per
// 32-cycle MFMA).  What the projections are of the encoder's time: DESIGN.md §4 "Latent cache".
// LDS images are As[k][m] / Bs[k][n] with the loader map of gemm.hip (kc_row / kc_k): conflict-free transposed writes,
// conflict-free fragment reads.
#include "common.h"

using namespace wfae;

typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));

namespace {

constexpr int RBM = 64, RBN = 64, RBK = 16, RNT = 256;
constexpr int RLD = 64 + 4;  // row stride of both LDS images: consecutive k-rows start four banks apart

template <int PREC, bool VEC>
__global__ __launch_bounds__(RNT) void linear_rowinv_kernel(const float* __restrict__ x, const float* __restrict__ w,
                                                            const float* __restrict__ bias, float* __restrict__ y, int B,
                                                            int In, int Out) {
  static_assert(RBM == RBN && RNT * 4 == RBM * RBK, "one float4 per thread, operand and stage");
  __shared__ float As[2][RBK][RLD];
  __shared__ float Bs[2][RBK][RLD];

  const int t = threadIdx.x;
  const int lane = t & 63, wave = t >> 6;
  const int l31 = lane & 31, lh = lane >> 5;
  const int m0 = blockIdx.x * RBM, n0 = blockIdx.y * RBN;
  const int wm0 = (wave >> 1) * 32, wn0 = (wave & 1) * 32;

  // loader: thread t owns the float4 (row lr, k = lk .. lk + 3) of both operand tiles
  const int lr = (t & 15) | ((t >> 6) << 4);
  const int lk = ((t >> 4) & 3) * 4;
  const bool a_ok = m0 + lr < B, b_ok = n0 + lr < Out;
  const float* ap = x + (long)(a_ok ? m0 + lr : 0) * In + lk;
  const float* bp = w + (long)(b_ok ? n0 + lr : 0) * In + lk;

  auto load = [&](const float* p, bool ok) -> float4 {
    float4 v;
    if constexpr (VEC)
      v = *reinterpret_cast<const float4*>(p);
    else
      v = make_float4(p[0], p[1], p[2], p[3]);
    return ok ? v : make_float4(0.f, 0.f, 0.f, 0.f);
  };
  auto store = [&](float (*S)[RLD], float4 v) {
    S[lk + 0][lr] = v.x;
    S[lk + 1][lr] = v.y;
    S[lk + 2][lr] = v.z;
    S[lk + 3][lr] = v.w;
  };

  f32x16 acc;
#pragma unroll
  for (int r = 0; r < 16; ++r) acc[r] = 0.f;

  const int nstages = In / RBK;
  float4 ra = load(ap, a_ok), rb = load(bp, b_ok);
  store(As[0], ra);
  store(Bs[0], rb);
  __syncthreads();
  for (int s = 0; s < nstages; ++s) {
    const int buf = s & 1;
    const bool more = s + 1 < nstages;
    if (more) {  // the next stage's global loads are in flight under this stage's MFMAs
      ap += RBK;
      bp += RBK;
      ra = load(ap, a_ok);
      rb = load(bp, b_ok);
    }
    if constexpr (PREC == WFAE_PRECISION_BF16) {
      bf16x8 a8, b8;
#pragma unroll
      for (int q = 0; q < 8; ++q) {
        a8[q] = (__bf16)As[buf][lh * 8 + q][wm0 + l31];
        b8[q] = (__bf16)Bs[buf][lh * 8 + q][wn0 + l31];
      }
      acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a8, b8, acc, 0, 0, 0);
    } else {
#pragma unroll
      for (int st = 0; st < RBK / 2; ++st) {
        const float a = As[buf][st * 2 + lh][wm0 + l31];
        const float b = Bs[buf][st * 2 + lh][wn0 + l31];
        acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a, b, acc, 0, 0, 0);
      }
    }
    if (more) {  // buffer buf ^ 1 was last read before the barrier that ended stage s - 1
      store(As[buf ^ 1], ra);
      store(Bs[buf ^ 1], rb);
    }
    __syncthreads();
  }

  // C/D layout of both instructions: column = lane & 31, row = (r & 3) + 8 (r >> 2) + 4 (lane >> 5)
  const int col = n0 + wn0 + l31;
  if (col >= Out) return;
  const float bv = bias ? bias[col] : 0.f;
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    const int row = m0 + wm0 + (r & 3) + 8 * (r >> 2) + 4 * lh;
    if (row < B) y[(long)row * Out + col] = bias ? acc[r] + bv : acc[r];
  }
}

template <int PREC>
void launch_rowinv(const float* x, const float* w, const float* bias, float* y, int B, int In, int Out, hipStream_t st) {
  const dim3 grid((B + RBM - 1) / RBM, (Out + RBN - 1) / RBN), block(RNT);
  // In % 32 == 0: every row starts 16-byte aligned when its base pointer does
  if ((((uintptr_t)x | (uintptr_t)w) & 15) == 0)
    hipLaunchKernelGGL((linear_rowinv_kernel<PREC, true>), grid, block, 0, st, x, w, bias, y, B, In, Out);
  else
    hipLaunchKernelGGL((linear_rowinv_kernel<PREC, false>), grid, block, 0, st, x, w, bias, y, B, In, Out);
}

}  // namespace

extern "C" {

int wfae_linear_fwd_rowinv(const float* x, const float* w, const float* bias, float* y, int B, int In, int Out,
                           wfae_stream_t stream) {
  WFAE_REQUIRE(x && w && y, WFAE_ERR_NULL_POINTER, "linear_fwd_rowinv: null pointer");
  WFAE_REQUIRE(B > 0 && In > 0 && Out > 0, WFAE_ERR_BAD_SHAPE, "linear_fwd_rowinv: bad shape B=%d In=%d Out=%d", B, In, Out);
  WFAE_REQUIRE(In % 32 == 0 && Out % 32 == 0 && In <= 4096 && Out <= 4096, WFAE_ERR_UNSUPPORTED,
               "linear_fwd_rowinv: In=%d Out=%d, served are multiples of 32 up to 4096", In, Out);
  if (wfae::matmul_precision() == WFAE_PRECISION_BF16)
    launch_rowinv<WFAE_PRECISION_BF16>(x, w, bias, y, B, In, Out, (hipStream_t)stream);
  else
    launch_rowinv<WFAE_PRECISION_FP32>(x, w, bias, y, B, In, Out, (hipStream_t)stream);
  return check_launch("linear_fwd_rowinv");
}

}  // extern "C"
