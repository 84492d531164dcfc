// lpips.hip — the LPIPS perceptual loss of the AE+GAN step (reference pipeline/models/autoencoderkl/losses/lpips.py `LPIPS`,
// `ScalingLayer`, `vgg16`, `normalize_tensor`, `spatial_average`): forward and the gradient with respect to the FIRST image.
// The VGG16 is frozen, so there are no weight gradients.  NCHW fp32, fixed summation order, no atomics: two launches give
// the same bits.
//
// conv3: the stride-1 pad-1 3x3 convolution of aekl.hip (`aekl_conv3_kernel` kind 0: same 64-channel x 8 x 16-pixel
//   workgroup tile, same LDS patch per 32-channel chunk, same packed weights — packed by wfae_aekl_conv3_pack —, same three
//   operand modes and the same two-level summation) without the GroupNorm prologue / residual / scale, with one of two
//   epilogues:
//     forward:        y  = max(conv + bias, 0)
//     backward-data:  dx = conv * (a_prev > 0)   over dy with the weights rotated 180 degrees and in / out transposed (the
//                     host packs w.flip(2, 3).transpose(0, 1) once); a_prev is the saved post-ReLU activation that fed the
//                     layer, so dx is the gradient of that activation's PRE-activation.  Null a_prev: no mask.
// pool: 2 x 2 stride 2 max-pool (floor).  Its backward writes the gradient of the pool input's pre-activation in one pass:
//   torch's routing (the first maximum of a window in the order (0,0), (0,1), (1,0), (1,1)), plus the distance gradient of
//   the same activation (every pool input is an LPIPS tap), times the ReLU mask.
// dist: one tap layer of the distance.  A workgroup owns 64 pixels of one sample; its four waves split the channels, the
//   four partial sums of a pixel are combined in LDS in a fixed order.  Per-thread sums are fp64.
// prep: ScalingLayer on a 1-channel (the reference's repeat(1, 3, 1, 1)) or 3-channel image.
#include "common.h"

using namespace wfae;

namespace {

typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef unsigned u32x4 __attribute__((ext_vector_type(4)));

constexpr int BM = 64;            // output channels of a workgroup
constexpr int TH = 8, TW = 16;    // output pixel tile
constexpr int CK = 32;            // input channels per chunk
constexpr int kThreads = 256;
constexpr int PH = TH + 2, PW = TW + 2, PP = PH * PW;   // the patch of a tile

enum { MODE_BF16 = 1, MODE_SPLIT3 = 3, MODE_F32 = 4 };
enum { EPI_RELU = 0, EPI_MASK = 1 };

struct L3P {
  const float* x;
  const void* w;
  const float* aux;   // EPI_RELU: bias (Cout);  EPI_MASK: a_prev (y's shape) or null
  float* y;
  int N, Cin, Cout, CoutP, H, W, nchunks, ncb;
};

// bytes of one pixel record: 32 channels + padding that spreads the 16 pixels of a fragment read over the banks
template <int MODE>
struct Rec {
  static constexpr int B = MODE == MODE_F32 ? 144 : 80;
};

template <int MODE, int EPI>
__global__ __launch_bounds__(kThreads) void lpips_conv3_kernel(L3P p) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  constexpr bool F32 = MODE == MODE_F32;
  constexpr int NP = F32 ? 1 : MODE;
  constexpr int REC = Rec<MODE>::B;
  constexpr int PLANE = PP * REC;
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6, r15 = lane & 15, g4 = lane >> 4;
  const int ox0 = blockIdx.x * TW, oy0 = blockIdx.y * TH;
  const int n = blockIdx.z / p.ncb, co0 = (blockIdx.z % p.ncb) * BM;
  const int HW = p.H * p.W;
  const float* __restrict__ xn = p.x + (long)n * p.Cin * HW;
  const long wplane = (long)p.nchunks * 9 * p.CoutP * CK;   // elements of one packed plane

  f32x4 acc[4][2];
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
      for (int q = 0; q < 4; ++q) acc[i][j][q] = 0.f;

  for (int cc = 0; cc < p.nchunks; ++cc) {
    // two-level summation (aekl.hip): the MFMAs of a chunk accumulate from zero, the chunk sums are added to the total
    f32x4 part[4][2];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
      for (int j = 0; j < 2; ++j)
#pragma unroll
        for (int q = 0; q < 4; ++q) part[i][j][q] = 0.f;
    __syncthreads();   // the fragment reads of the previous chunk are done
    // ---- stage the patch: item = (pixel, group of 8 channels); lanes run along the pixels
    for (int it = t; it < PP * 4; it += kThreads) {
      const int pix = it % PP, g = it / PP;
      const int py = pix / PW, px = pix - py * PW;
      const int sy = oy0 - 1 + py, sx = ox0 - 1 + px;
      const bool ok = sy >= 0 && sy < p.H && sx >= 0 && sx < p.W;
      const int c0 = cc * CK + g * 8;
      float v[8];
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const int ci = c0 + j;
        v[j] = (ok && ci < p.Cin) ? xn[(long)ci * HW + sy * p.W + sx] : 0.f;   // padding pixels and padding channels
      }
      unsigned char* dst = smem + pix * REC + g * (F32 ? 32 : 16);
      if (F32) {
        *reinterpret_cast<f32x4*>(dst) = f32x4{v[0], v[1], v[2], v[3]};
        *reinterpret_cast<f32x4*>(dst + 16) = f32x4{v[4], v[5], v[6], v[7]};
      } else if (NP == 1) {
        *reinterpret_cast<u32x4*>(dst) = u32x4{pack_bf16(v[0], v[1]), pack_bf16(v[2], v[3]), pack_bf16(v[4], v[5]), pack_bf16(v[6], v[7])};
      } else {
        unsigned short h[8], m[8], l[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) split3(v[j], h[j], m[j], l[j]);
#define WFAE_PK(a, j) ((unsigned)a[j] | ((unsigned)a[j + 1] << 16))
        *reinterpret_cast<u32x4*>(dst) = u32x4{WFAE_PK(h, 0), WFAE_PK(h, 2), WFAE_PK(h, 4), WFAE_PK(h, 6)};
        *reinterpret_cast<u32x4*>(dst + PLANE) = u32x4{WFAE_PK(m, 0), WFAE_PK(m, 2), WFAE_PK(m, 4), WFAE_PK(m, 6)};
        *reinterpret_cast<u32x4*>(dst + 2 * PLANE) = u32x4{WFAE_PK(l, 0), WFAE_PK(l, 2), WFAE_PK(l, 4), WFAE_PK(l, 6)};
#undef WFAE_PK
      }
    }
    __syncthreads();

    // ---- nine taps: shifted fragment reads of the same patch
#pragma unroll
    for (int tap = 0; tap < 9; ++tap) {
      const int ky = tap / 3, kx = tap % 3;
      const long wrow = ((long)(cc * 9 + tap) * p.CoutP + co0 + r15) * CK;   // + 16 i * CK
      if constexpr (!F32) {
        const unsigned short* __restrict__ wp = reinterpret_cast<const unsigned short*>(p.w);
        bf16x8 a[4][NP], b[2][NP];
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
          for (int pl = 0; pl < NP; ++pl)
            a[i][pl] = *reinterpret_cast<const bf16x8*>(wp + pl * wplane + wrow + 16 * i * CK + 8 * g4);
#pragma unroll
        for (int j = 0; j < 2; ++j) {
          const int pix = (2 * wave + j + ky) * PW + r15 + kx;
#pragma unroll
          for (int pl = 0; pl < NP; ++pl)
            b[j][pl] = *reinterpret_cast<const bf16x8*>(smem + pl * PLANE + pix * REC + 16 * g4);
        }
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
          for (int j = 0; j < 2; ++j) {
            f32x4 c = part[i][j];   // smallest terms first
            if constexpr (NP == 3) {
              c = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a[i][2], b[j][0], c, 0, 0, 0);
              c = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a[i][0], b[j][2], c, 0, 0, 0);
              c = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a[i][1], b[j][1], c, 0, 0, 0);
              c = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a[i][1], b[j][0], c, 0, 0, 0);
              c = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a[i][0], b[j][1], c, 0, 0, 0);
            }
            c = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a[i][0], b[j][0], c, 0, 0, 0);
            part[i][j] = c;
          }
      } else {
        // the MFMA's k index is the lane group g4; in sub-step (hf, c) it stands for channel 16 hf + 4 g4 + c on both sides
        const float* __restrict__ wp = reinterpret_cast<const float*>(p.w);
#pragma unroll
        for (int hf = 0; hf < 2; ++hf) {
          f32x4 a[4], b[2];
#pragma unroll
          for (int i = 0; i < 4; ++i) a[i] = *reinterpret_cast<const f32x4*>(wp + wrow + 16 * i * CK + 16 * hf + 4 * g4);
#pragma unroll
          for (int j = 0; j < 2; ++j) {
            const int pix = (2 * wave + j + ky) * PW + r15 + kx;
            b[j] = *reinterpret_cast<const f32x4*>(smem + pix * REC + 64 * hf + 16 * g4);
          }
#pragma unroll
          for (int c = 0; c < 4; ++c)
#pragma unroll
            for (int i = 0; i < 4; ++i)
#pragma unroll
              for (int j = 0; j < 2; ++j)
                part[i][j] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[i][c], b[j][c], part[i][j], 0, 0, 0);
        }
      }
    }
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
      for (int j = 0; j < 2; ++j) acc[i][j] += part[i][j];
  }

  // ---- epilogue: accumulator register q of lane (r15, g4) is (co = 16 i + 4 g4 + q, pixel r15 of tile row 2 wave + j)
  const int ox = ox0 + r15;
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    const int oy = oy0 + 2 * wave + j;
    if (oy >= p.H || ox >= p.W) continue;
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const int co = co0 + 16 * i + 4 * g4 + q;
        if (co >= p.Cout) continue;
        const long o = ((long)n * p.Cout + co) * HW + oy * p.W + ox;
        float v = acc[i][j][q];
        if constexpr (EPI == EPI_RELU) {
          v = fmaxf(v + p.aux[co], 0.f);
        } else {
          if (p.aux && !(p.aux[o] > 0.f)) v = 0.f;
        }
        p.y[o] = v;
      }
  }
}

__global__ __launch_bounds__(256) void lpips_pool_fwd_kernel(const float* __restrict__ x, float* __restrict__ y, int H, int W,
                                                             int Ho, int Wo, long total) {
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= total) return;
  const int ox = (int)(i % Wo);
  const long r = i / Wo;
  const int oy = (int)(r % Ho);
  const long nc = r / Ho;
  const float* __restrict__ s = x + nc * H * W + (long)(2 * oy) * W + 2 * ox;
  y[i] = fmaxf(fmaxf(s[0], s[1]), fmaxf(s[W], s[W + 1]));
}

// one thread per element of the pool's INPUT
__global__ __launch_bounds__(256) void lpips_pool_bwd_kernel(const float* __restrict__ a, const float* __restrict__ dy,
                                                             const float* __restrict__ add, float* __restrict__ dpre, int H,
                                                             int W, int Ho, int Wo, long total) {
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= total) return;
  const int x = (int)(i % W);
  const long r = i / W;
  const int y = (int)(r % H);
  const long nc = r / H;
  const float v = a[i];
  float g = add ? add[i] : 0.f;
  const int oy = y >> 1, ox = x >> 1;
  if (oy < Ho && ox < Wo) {
    const float* __restrict__ s = a + nc * H * W + (long)(2 * oy) * W + 2 * ox;
    const float w4[4] = {s[0], s[1], s[W], s[W + 1]};
    const int me = 2 * (y & 1) + (x & 1);
    bool first = true;   // v is the window's maximum and no earlier element equals it
#pragma unroll
    for (int k = 0; k < 4; ++k) first = first && (k < me ? w4[k] < v : w4[k] <= v);
    if (first) g += dy[(nc * Ho + oy) * Wo + ox];
  }
  dpre[i] = v > 0.f ? g : 0.f;
}

constexpr int kDistPix = 64;      // pixels of a workgroup; its 4 waves split the channels
constexpr float kDistEps = 1e-10f;

// the four channel-group partials of pixel px, combined in a fixed order
__device__ __forceinline__ double dist_combine(const double (*sh)[kDistPix], int px) {
  return (sh[0][px] + sh[1][px]) + (sh[2][px] + sh[3][px]);
}

// ||a0||, ||a1|| over the channels of this thread's pixel (every thread of the workgroup gets them)
__device__ __forceinline__ void dist_norms(const float* __restrict__ p0, const float* __restrict__ p1, bool ok, int c_lo, int c_hi,
                                           long HW, double (*sh)[4][kDistPix], int px, int cg, float& k0, float& k1) {
  double s0 = 0.0, s1 = 0.0;
  if (ok)
    for (int c = c_lo; c < c_hi; ++c) {
      const double v0 = p0[c * HW], v1 = p1[c * HW];
      s0 = fma(v0, v0, s0);
      s1 = fma(v1, v1, s1);
    }
  sh[0][cg][px] = s0;
  sh[1][cg][px] = s1;
  __syncthreads();
  k0 = sqrtf((float)dist_combine(sh[0], px));
  k1 = sqrtf((float)dist_combine(sh[1], px));
  __syncthreads();
}

// part[n][blk] = sum over the block's pixels of sum_c lin[c] (a0 / (||a0|| + eps) - a1 / (||a1|| + eps))^2
__global__ __launch_bounds__(256) void lpips_dist_part_kernel(const float* __restrict__ a0, const float* __restrict__ a1,
                                                              const float* __restrict__ lin, double* __restrict__ part, int C,
                                                              long HW, int nblk) {
  __shared__ double sh[2][4][kDistPix];
  const int px = threadIdx.x & 63, cg = threadIdx.x >> 6, n = blockIdx.y;
  const long pix = (long)blockIdx.x * kDistPix + px;
  const bool ok = pix < HW;
  const float* __restrict__ p0 = a0 + (long)n * C * HW + pix;
  const float* __restrict__ p1 = a1 + (long)n * C * HW + pix;
  const int c_lo = cg * (C / 4), c_hi = c_lo + C / 4;
  float k0, k1;
  dist_norms(p0, p1, ok, c_lo, c_hi, HW, sh, px, cg, k0, k1);
  const float q0 = k0 + kDistEps, q1 = k1 + kDistEps;
  double s = 0.0;
  if (ok)
    for (int c = c_lo; c < c_hi; ++c) {
      const float d = p0[c * HW] / q0 - p1[c * HW] / q1;
      s = fma((double)lin[c], (double)(d * d), s);
    }
  sh[0][cg][px] = s;
  __syncthreads();
  if (cg == 0) {
    const double tot = wave_sum(dist_combine(sh[0], px));
    if (px == 0) part[(long)n * nblk + blockIdx.x] = tot;
  }
}

// out[n] += sum of the sample's partials / HW
__global__ __launch_bounds__(256) void lpips_dist_final_kernel(const double* __restrict__ part, float* __restrict__ out, int nblk,
                                                               long HW) {
  __shared__ double red[16];
  const int n = blockIdx.x;
  double s = 0.0;
  for (int b = threadIdx.x; b < nblk; b += 256) s += part[(long)n * nblk + b];
  s = block_sum(s, red);
  if (threadIdx.x == 0) out[n] += (float)(s / (double)HW);
}

// da0 of the sample's term g[n] / HW * sum_pixels sum_c lin[c] (f0 - f1)^2.  With u_c = 2 g / HW lin_c (f0_c - f1_c) and
// q = ||a0|| + eps:  da0_j = u_j / q - (a0_j / ||a0||) (sum_c u_c a0_c) / q^2; the second term is dropped where ||a0|| == 0
// (the reference's autograd gives 0 * inf = NaN there).  relu != 0: times (a0 > 0).
__global__ __launch_bounds__(256) void lpips_dist_bwd_kernel(const float* __restrict__ a0, const float* __restrict__ a1,
                                                             const float* __restrict__ lin, const float* __restrict__ g,
                                                             float* __restrict__ da0, int C, long HW, int relu) {
  __shared__ double sh[2][4][kDistPix];
  const int px = threadIdx.x & 63, cg = threadIdx.x >> 6, n = blockIdx.y;
  const long pix = (long)blockIdx.x * kDistPix + px;
  const bool ok = pix < HW;
  const float* __restrict__ p0 = a0 + (long)n * C * HW + pix;
  const float* __restrict__ p1 = a1 + (long)n * C * HW + pix;
  float* __restrict__ pd = da0 + (long)n * C * HW + pix;
  const int c_lo = cg * (C / 4), c_hi = c_lo + C / 4;
  float k0, k1;
  dist_norms(p0, p1, ok, c_lo, c_hi, HW, sh, px, cg, k0, k1);
  const float q0 = k0 + kDistEps, q1 = k1 + kDistEps;
  const float coef = 2.0f * g[n] / (float)HW;
  double s = 0.0;
  if (ok)
    for (int c = c_lo; c < c_hi; ++c) {
      const float v0 = p0[c * HW];
      const float u = coef * lin[c] * (v0 / q0 - p1[c * HW] / q1);
      s = fma((double)u, (double)v0, s);
    }
  sh[0][cg][px] = s;
  __syncthreads();
  const float proj = k0 > 0.f ? (float)(dist_combine(sh[0], px) / ((double)q0 * (double)q0)) / k0 : 0.f;
  if (ok)
    for (int c = c_lo; c < c_hi; ++c) {
      const float v0 = p0[c * HW];
      const float u = coef * lin[c] * (v0 / q0 - p1[c * HW] / q1);
      const float d = u / q0 - v0 * proj;
      pd[c * HW] = (relu && !(v0 > 0.f)) ? 0.f : d;
    }
}

// y[n][c] = (x[n][c or 0] - shift[c]) / scale[c], c < 3
__global__ __launch_bounds__(256) void lpips_prep_fwd_kernel(const float* __restrict__ x, const float* __restrict__ shift,
                                                             const float* __restrict__ scale, float* __restrict__ y, int Cx,
                                                             long HW, long total) {
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= total) return;
  const long n = i / HW, p = i - n * HW;
#pragma unroll
  for (int c = 0; c < 3; ++c) y[(n * 3 + c) * HW + p] = (x[(n * Cx + (Cx == 3 ? c : 0)) * HW + p] - shift[c]) / scale[c];
}

__global__ __launch_bounds__(256) void lpips_prep_bwd_kernel(const float* __restrict__ dy, const float* __restrict__ scale,
                                                             float* __restrict__ dx, int Cx, long HW, long total) {
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= total) return;
  const long n = i / HW, p = i - n * HW;
  float d[3];
#pragma unroll
  for (int c = 0; c < 3; ++c) d[c] = dy[(n * 3 + c) * HW + p] / scale[c];
  if (Cx == 3) {
#pragma unroll
    for (int c = 0; c < 3; ++c) dx[(n * 3 + c) * HW + p] = d[c];
  } else {
    dx[i] = (d[0] + d[1]) + d[2];
  }
}

inline bool mode_ok(int mode) { return mode == MODE_BF16 || mode == MODE_SPLIT3 || mode == MODE_F32; }
inline int pad_to(int v, int m) { return (v + m - 1) / m * m; }
inline unsigned blocks_of(long total) { return (unsigned)((total + 255) / 256); }

template <int MODE, int EPI>
int launch_conv3(const L3P& p, hipStream_t st, const char* what) {
  constexpr size_t lds = (size_t)PP * Rec<MODE>::B * (MODE == MODE_SPLIT3 ? 3 : 1);
  static_assert(lds <= 64 * 1024, "patch does not fit LDS");
  const dim3 grid(cdiv(p.W, TW), cdiv(p.H, TH), p.N * p.ncb);
  hipLaunchKernelGGL((lpips_conv3_kernel<MODE, EPI>), grid, dim3(kThreads), lds, st, p);
  return check_launch(what);
}

// the checks and the launch shared by the two conv entry points; (Cin, Cout) in the GEMM's sense: x has Cin channels
template <int EPI>
int conv3(const char* what, const float* x, const void* packed, const float* aux, float* y, int mode, int N, int Cin, int Cout,
          int H, int W, wfae_stream_t stream) {
  WFAE_REQUIRE(x && packed && y && (EPI == EPI_MASK || aux), WFAE_ERR_NULL_POINTER, "%s: null pointer", what);
  WFAE_REQUIRE(mode_ok(mode), WFAE_ERR_BAD_SHAPE, "%s: mode %d (1 = bf16, 3 = three bf16 planes, 4 = fp32)", what, mode);
  WFAE_REQUIRE(N > 0 && H > 0 && W > 0 && H <= 8192 && W <= 8192, WFAE_ERR_BAD_SHAPE, "%s: bad shape N=%d H=%d W=%d", what, N, H, W);
  WFAE_REQUIRE(Cout > 0 && Cin > 0 && Cout <= 4096 && Cin <= 4096, WFAE_ERR_UNSUPPORTED,
               "%s: channel counts 1..4096 are served (got %d and %d)", what, Cin, Cout);
  WFAE_REQUIRE((reinterpret_cast<uintptr_t>(packed) & 15) == 0, WFAE_ERR_BAD_SHAPE, "%s: packed must be 16-byte aligned", what);
  L3P p = {};
  p.x = x; p.w = packed; p.aux = aux; p.y = y;
  p.N = N; p.Cin = Cin; p.Cout = Cout; p.H = H; p.W = W;
  p.CoutP = pad_to(Cout, BM);
  p.ncb = p.CoutP / BM;
  p.nchunks = pad_to(Cin, CK) / CK;
  WFAE_REQUIRE((long)Cin * H * W < (1l << 31) && (long)Cout * H * W < (1l << 31), WFAE_ERR_BAD_SHAPE,
               "%s: one sample must stay below 2^31 elements", what);
  WFAE_REQUIRE((long)N * p.ncb <= 65535 && cdiv(H, TH) <= 65535, WFAE_ERR_BAD_SHAPE, "%s: grid too large", what);
  hipStream_t st = (hipStream_t)stream;
  if (mode == MODE_BF16) return launch_conv3<MODE_BF16, EPI>(p, st, what);
  if (mode == MODE_SPLIT3) return launch_conv3<MODE_SPLIT3, EPI>(p, st, what);
  return launch_conv3<MODE_F32, EPI>(p, st, what);
}

inline bool dist_channels_ok(int C) { return C == 64 || C == 128 || C == 256 || C == 512; }

}  // namespace

extern "C" {

int wfae_lpips_conv3_fwd(const float* x, const void* packed, const float* bias, float* y, int mode, int N, int Cin, int Cout,
                         int H, int W, wfae_stream_t stream) {
  return conv3<EPI_RELU>("lpips_conv3_fwd", x, packed, bias, y, mode, N, Cin, Cout, H, W, stream);
}

int wfae_lpips_conv3_bwd_data(const float* dy, const void* packed_t, const float* a_prev, float* dx, int mode, int N, int Cin,
                              int Cout, int H, int W, wfae_stream_t stream) {
  return conv3<EPI_MASK>("lpips_conv3_bwd_data", dy, packed_t, a_prev, dx, mode, N, Cout, Cin, H, W, stream);
}

int wfae_lpips_pool_fwd(const float* x, float* y, int N, int C, int H, int W, wfae_stream_t stream) {
  WFAE_REQUIRE(x && y, WFAE_ERR_NULL_POINTER, "lpips_pool_fwd: null pointer");
  WFAE_REQUIRE(N > 0 && C > 0 && H >= 2 && W >= 2 && (long)H * W < (1l << 31), WFAE_ERR_BAD_SHAPE,
               "lpips_pool_fwd: bad shape N=%d C=%d H=%d W=%d (a plane of at least 2x2)", N, C, H, W);
  const int Ho = H / 2, Wo = W / 2;
  const long total = (long)N * C * Ho * Wo;
  WFAE_REQUIRE((long)N * C * H * W < (1l << 39), WFAE_ERR_BAD_SHAPE, "lpips_pool_fwd: too large");
  hipLaunchKernelGGL(lpips_pool_fwd_kernel, dim3(blocks_of(total)), dim3(256), 0, (hipStream_t)stream, x, y, H, W, Ho, Wo, total);
  return check_launch("lpips_pool_fwd");
}

int wfae_lpips_pool_bwd(const float* a, const float* dy, const float* add, float* dpre, int N, int C, int H, int W,
                        wfae_stream_t stream) {
  WFAE_REQUIRE(a && dy && dpre, WFAE_ERR_NULL_POINTER, "lpips_pool_bwd: null pointer");
  WFAE_REQUIRE(N > 0 && C > 0 && H >= 2 && W >= 2 && (long)H * W < (1l << 31), WFAE_ERR_BAD_SHAPE,
               "lpips_pool_bwd: bad shape N=%d C=%d H=%d W=%d (a plane of at least 2x2)", N, C, H, W);
  const long total = (long)N * C * H * W;
  WFAE_REQUIRE(total < (1l << 39), WFAE_ERR_BAD_SHAPE, "lpips_pool_bwd: too large");
  hipLaunchKernelGGL(lpips_pool_bwd_kernel, dim3(blocks_of(total)), dim3(256), 0, (hipStream_t)stream, a, dy, add, dpre, H, W,
                     H / 2, W / 2, total);
  return check_launch("lpips_pool_bwd");
}

size_t wfae_lpips_dist_ws_bytes(int N, int HW) {
  if (N <= 0 || HW <= 0) return 0;
  return (size_t)N * cdiv(HW, kDistPix) * sizeof(double);
}

int wfae_lpips_dist_fwd(const float* a0, const float* a1, const float* lin, float* out, int N, int C, int HW, void* ws,
                        size_t ws_bytes, wfae_stream_t stream) {
  WFAE_REQUIRE(a0 && a1 && lin && out, WFAE_ERR_NULL_POINTER, "lpips_dist_fwd: null pointer");
  WFAE_REQUIRE(N > 0 && N <= 65535 && HW > 0, WFAE_ERR_BAD_SHAPE, "lpips_dist_fwd: bad shape N=%d HW=%d", N, HW);
  WFAE_REQUIRE(dist_channels_ok(C), WFAE_ERR_UNSUPPORTED, "lpips_dist_fwd: C = %d, served are 64, 128, 256, 512", C);
  const size_t need = wfae_lpips_dist_ws_bytes(N, HW);
  WFAE_REQUIRE(ws && ws_bytes >= need, WFAE_ERR_WORKSPACE, "lpips_dist_fwd: workspace too small (%zu < %zu)", ws_bytes, need);
  WFAE_REQUIRE((reinterpret_cast<uintptr_t>(ws) & 7) == 0, WFAE_ERR_WORKSPACE, "lpips_dist_fwd: workspace must be 8-byte aligned");
  const int nblk = cdiv(HW, kDistPix);
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(lpips_dist_part_kernel, dim3(nblk, N), dim3(256), 0, st, a0, a1, lin, (double*)ws, C, (long)HW, nblk);
  int rc = check_launch("lpips_dist_part");
  if (rc) return rc;
  hipLaunchKernelGGL(lpips_dist_final_kernel, dim3(N), dim3(256), 0, st, (const double*)ws, out, nblk, (long)HW);
  return check_launch("lpips_dist_final");
}

int wfae_lpips_dist_bwd(const float* a0, const float* a1, const float* lin, const float* g, float* da0, int N, int C, int HW,
                        int relu, wfae_stream_t stream) {
  WFAE_REQUIRE(a0 && a1 && lin && g && da0, WFAE_ERR_NULL_POINTER, "lpips_dist_bwd: null pointer");
  WFAE_REQUIRE(N > 0 && N <= 65535 && HW > 0, WFAE_ERR_BAD_SHAPE, "lpips_dist_bwd: bad shape N=%d HW=%d", N, HW);
  WFAE_REQUIRE(dist_channels_ok(C), WFAE_ERR_UNSUPPORTED, "lpips_dist_bwd: C = %d, served are 64, 128, 256, 512", C);
  hipLaunchKernelGGL(lpips_dist_bwd_kernel, dim3(cdiv(HW, kDistPix), N), dim3(256), 0, (hipStream_t)stream, a0, a1, lin, g, da0, C,
                     (long)HW, relu);
  return check_launch("lpips_dist_bwd");
}

int wfae_lpips_prep_fwd(const float* x, const float* shift, const float* scale, float* y, int N, int Cx, int HW,
                        wfae_stream_t stream) {
  WFAE_REQUIRE(x && shift && scale && y, WFAE_ERR_NULL_POINTER, "lpips_prep_fwd: null pointer");
  WFAE_REQUIRE(N > 0 && HW > 0, WFAE_ERR_BAD_SHAPE, "lpips_prep_fwd: bad shape N=%d HW=%d", N, HW);
  WFAE_REQUIRE(Cx == 1 || Cx == 3, WFAE_ERR_UNSUPPORTED, "lpips_prep_fwd: %d input channels, served are 1 and 3", Cx);
  const long total = (long)N * HW;
  hipLaunchKernelGGL(lpips_prep_fwd_kernel, dim3(blocks_of(total)), dim3(256), 0, (hipStream_t)stream, x, shift, scale, y, Cx,
                     (long)HW, total);
  return check_launch("lpips_prep_fwd");
}

int wfae_lpips_prep_bwd(const float* dy, const float* scale, float* dx, int N, int Cx, int HW, wfae_stream_t stream) {
  WFAE_REQUIRE(dy && scale && dx, WFAE_ERR_NULL_POINTER, "lpips_prep_bwd: null pointer");
  WFAE_REQUIRE(N > 0 && HW > 0, WFAE_ERR_BAD_SHAPE, "lpips_prep_bwd: bad shape N=%d HW=%d", N, HW);
  WFAE_REQUIRE(Cx == 1 || Cx == 3, WFAE_ERR_UNSUPPORTED, "lpips_prep_bwd: %d input channels, served are 1 and 3", Cx);
  const long total = (long)N * HW;
  hipLaunchKernelGGL(lpips_prep_bwd_kernel, dim3(blocks_of(total)), dim3(256), 0, (hipStream_t)stream, dy, scale, dx, Cx, (long)HW,
                     total);
  return check_launch("lpips_prep_bwd");
}

}  // extern "C"
