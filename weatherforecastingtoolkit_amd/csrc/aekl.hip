// aekl.hip — forward kernels of the frozen AutoencoderKL latent provider (reference pipeline/models/autoencoderkl/
// autoencoder_kl.py `AutoencoderKL`, vae.py `Encoder` / `Decoder`, resnet.py `ResnetBlock2D` / `Downsample2D` / `Upsample2D`,
// attention.py `AttentionBlock`, distributions.py `DiagonalGaussianDistribution`).
//
// conv3: the 3x3 convolution as an implicit GEMM on the matrix cores, NCHW fp32 in and out, fp32 accumulation.
//   kind 0: stride 1, pad 1.   kind 1: stride 2 over the input padded (0, 1, 0, 1) (Downsample2D with padding = 0).
//   kind 2: stride 1, pad 1 over the nearest-neighbour x2 upsample of the input (Upsample2D + conv); the 4x tensor is
//   never written, the loader reads source pixel (uy >> 1, ux >> 1).
//   A workgroup of 4 waves owns 64 output channels x an 8 x 16 output pixel tile.  Per 32-input-channel chunk it stages the
//   input patch of the tile ((8 + 2) x (16 + 2) pixels; 17 x 33 for stride 2) in LDS as [pixel][32 channels], ONCE for all
//   nine taps: the optional prologue SiLU(x * scale[n, c] + shift[n, c]) (GroupNorm folded by gn_stats) runs here, and
//   padding pixels are stored as literal zeros AFTER it (silu(gn(0)) != 0).  A tap is then a shifted read of the same
//   patch: B fragments come from LDS (16 pixels of one output row x 32 channels), A fragments straight from the packed
//   weights in global memory ([chunk][tap][co][32 ci]: one 16-byte read per lane, the same for every workgroup of the layer,
//   so they live in L2 / the vector cache).
//   mode 3: every operand is carried as three bf16 planes (x == h + m + l exactly, split once at the LDS store / at pack
//   time) and a product is six v_mfma_f32_16x16x32_bf16 — the split GEMMs' arithmetic (splitgemm.hip).  mode 1: the h
//   plane alone (operands rounded to bf16: 'medium').  mode 4: fp32 operands on v_mfma_f32_16x16x4_f32.
//   The MFMAs of a chunk accumulate from zero and the chunk sums are added up (two-level summation).
//   Epilogue: + bias, + residual, * out_mul.  Channel counts are padded to 32 (input, zeros) / 64 (output, not stored).
//   Fixed summation order, no atomics: two launches give the same bits.
// gn_stats: GroupNorm statistics, two levels, fixed order: per slice (mean, M2) taken in two passes over the slice, slices
//   combined pairwise-exactly (Chan et al.) in fp64 — never E[x^2] - E[x]^2.  Writes mean / rstd per (sample, group) and
//   the folded scale = gamma rstd, shift = beta - mean rstd gamma per (sample, channel).
// tokens / softmax: the pieces of the single-head mid-block attention that linear_fwd and split_gemm do not cover.
// posterior: DiagonalGaussianDistribution from the quant_conv moments.
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
constexpr size_t kLdsLimit = 160 * 1024;

enum { MODE_BF16 = 1, MODE_SPLIT3 = 3, MODE_F32 = 4 };

struct C3P {
  const float* x;
  const void* w;
  const float* bias;
  const float* gscale;
  const float* gshift;
  const float* res;
  float* y;
  int N, Cin, Cout, CoutP, H, W, Ho, Wo, nchunks, ncb;
  float out_mul;
};

template <int KIND>
struct Geo {
  static constexpr int S = KIND == 1 ? 2 : 1;
  static constexpr int PH = S * (TH - 1) + 3, PW = S * (TW - 1) + 3, PP = PH * PW;
};
// bytes of one pixel record: 32 channels + padding that spreads the 16 pixels of a fragment read over the banks
template <int MODE>
struct Rec {
  static constexpr int B = MODE == MODE_F32 ? 144 : 80;
};

__device__ __forceinline__ float silu_f(float v) { return v / (1.0f + expf(-v)); }

template <int KIND, int MODE>
__global__ __launch_bounds__(kThreads) void aekl_conv3_kernel(C3P p) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  constexpr bool F32 = MODE == MODE_F32;
  constexpr int NP = F32 ? 1 : MODE;
  constexpr int S = Geo<KIND>::S, PW = Geo<KIND>::PW, PP = Geo<KIND>::PP;
  constexpr int REC = Rec<MODE>::B;
  constexpr int PLANE = PP * REC;
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6, r15 = lane & 15, g4 = lane >> 4;
  const int ox0 = blockIdx.x * TW, oy0 = blockIdx.y * TH;
  const int n = blockIdx.z / p.ncb, co0 = (blockIdx.z % p.ncb) * BM;
  const int HW = p.H * p.W;
  const float* __restrict__ xn = p.x + (long)n * p.Cin * HW;
  const bool pro = p.gscale != nullptr;
  const float* __restrict__ gs = pro ? p.gscale + (long)n * p.Cin : nullptr;
  const float* __restrict__ gh = pro ? p.gshift + (long)n * p.Cin : nullptr;
  const long wplane = (long)p.nchunks * 9 * p.CoutP * CK;   // elements of one packed plane

  f32x4 acc[4][2];
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
      for (int q = 0; q < 4; ++q) acc[i][j][q] = 0.f;

  for (int cc = 0; cc < p.nchunks; ++cc) {
    // two-level summation: the 54 (split) or 72 (fp32) MFMAs of a chunk accumulate from zero and the chunk sums are added
    // to the total.  One chain over all of K = 9 Cin (864 accumulations at Cin = 512) lost about 2e-6 of max |y|, three
    // times what torch's blocked CPU convolution loses; with the chunk level the error is sqrt(n / 2) eps for n = 54 and 16
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
      int sy, sx;
      bool ok;
      if (KIND == 0) {
        sy = oy0 - 1 + py; sx = ox0 - 1 + px;
        ok = sy >= 0 && sy < p.H && sx >= 0 && sx < p.W;
      } else if (KIND == 1) {
        sy = 2 * oy0 + py; sx = 2 * ox0 + px;
        ok = sy < p.H && sx < p.W;
      } else {
        const int uy = oy0 - 1 + py, ux = ox0 - 1 + px;
        ok = uy >= 0 && uy < 2 * p.H && ux >= 0 && ux < 2 * p.W;
        sy = uy >> 1; sx = ux >> 1;
      }
      const int c0 = cc * CK + g * 8;
      float v[8];
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const int ci = c0 + j;
        float val = 0.f;   // padding pixels and padding channels: zero after the prologue
        if (ok && ci < p.Cin) {
          val = xn[(long)ci * HW + sy * p.W + sx];
          if (pro) val = silu_f(fmaf(val, gs[ci], gh[ci]));
        }
        v[j] = val;
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
          const int pix = (S * (2 * wave + j) + ky) * PW + S * r15 + kx;
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
            const int pix = (S * (2 * wave + j) + ky) * PW + S * r15 + kx;
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
  const int HWo = p.Ho * p.Wo;
  const int ox = ox0 + r15;
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    const int oy = oy0 + 2 * wave + j;
    if (oy >= p.Ho || ox >= p.Wo) continue;
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const int co = co0 + 16 * i + 4 * g4 + q;
        if (co >= p.Cout) continue;
        const long o = ((long)n * p.Cout + co) * HWo + oy * p.Wo + ox;
        float v = acc[i][j][q];
        if (p.bias) v += p.bias[co];
        if (p.res) v += p.res[o];
        p.y[o] = v * p.out_mul;
      }
  }
}

// packed[plane][chunk][tap][co < CoutP][32 ci]; zeros in the channel padding
template <bool F32>
__global__ __launch_bounds__(256) void aekl_pack_kernel(const float* __restrict__ w, void* __restrict__ out, int Cout, int Cin,
                                                        int CoutP, int nchunks, int planes) {
  const long total = (long)nchunks * 9 * CoutP * CK;
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= total) return;
  const int k = (int)(i % CK);
  const long r = i / CK;
  const int co = (int)(r % CoutP);
  const int ct = (int)(r / CoutP), tap = ct % 9, cc = ct / 9;
  const int ci = cc * CK + k;
  const float v = (co < Cout && ci < Cin) ? w[((long)co * Cin + ci) * 9 + tap] : 0.f;
  if (F32) {
    reinterpret_cast<float*>(out)[i] = v;
  } else {
    unsigned short h, m, l;
    split3(v, h, m, l);
    unsigned short* o = reinterpret_cast<unsigned short*>(out);
    o[i] = h;
    if (planes == 3) {
      o[total + i] = m;
      o[2 * total + i] = l;
    }
  }
}

constexpr int kGnSlice = 16384;   // elements of a group one workgroup reduces

// level 1: (mean, M2) of slice blockIdx.x of group blockIdx.y (a group of NCHW is one contiguous span of L floats)
__global__ __launch_bounds__(256) void aekl_gn_part_kernel(const float* __restrict__ x, double* __restrict__ part, long L,
                                                           int nblk) {
  __shared__ double red[16];
  __shared__ double bc;
  const long b0 = (long)blockIdx.x * kGnSlice;
  const int cnt = (int)min((long)kGnSlice, L - b0);
  const float* __restrict__ xs = x + (long)blockIdx.y * L + b0;
  float s = 0.f;
  for (int i = threadIdx.x; i < cnt; i += 256) s += xs[i];
  const double mu = block_sum_all((double)s, red, &bc) / (double)cnt;
  const float muf = (float)mu;
  float q = 0.f;
  for (int i = threadIdx.x; i < cnt; i += 256) {
    const float d = xs[i] - muf;
    q = fmaf(d, d, q);
  }
  const double m2 = block_sum_all((double)q, red, &bc);
  if (threadIdx.x == 0) {
    // M2 about the exact slice mean mu, from the sum about its fp32 rounding muf
    const double dm = (double)muf - mu;
    double* o = part + ((long)blockIdx.y * nblk + blockIdx.x) * 2;
    o[0] = mu;
    o[1] = m2 - (double)cnt * dm * dm;
  }
}

// level 2: one workgroup per (sample, group): slices combined in ascending order, then the folded affine of its channels
__global__ __launch_bounds__(64) void aekl_gn_final_kernel(const double* __restrict__ part, const float* __restrict__ gamma,
                                                           const float* __restrict__ beta, float* __restrict__ mean,
                                                           float* __restrict__ rstd, float* __restrict__ scale,
                                                           float* __restrict__ shift, long L, int nblk, int C, int G,
                                                           float eps) {
  __shared__ float sm[2];
  const int ng = blockIdx.x, n = ng / G, g = ng % G, Cg = C / G;
  if (threadIdx.x == 0) {
    const double* pp = part + (long)ng * nblk * 2;
    double na = 0.0, ma = 0.0, M2 = 0.0;
    for (int b = 0; b < nblk; ++b) {
      const double nb = (double)min((long)kGnSlice, L - (long)b * kGnSlice);
      const double d = pp[2 * b] - ma, nt = na + nb;
      ma += d * nb / nt;
      M2 += pp[2 * b + 1] + d * d * na * nb / nt;
      na = nt;
    }
    double var = M2 / (double)L;
    if (var < 0.0) var = 0.0;
    const float mu = (float)ma, rs = (float)(1.0 / sqrt(var + (double)eps));
    mean[ng] = mu;
    rstd[ng] = rs;
    sm[0] = mu;
    sm[1] = rs;
  }
  __syncthreads();
  const float mu = sm[0], rs = sm[1];
  for (int c = threadIdx.x; c < Cg; c += 64) {
    const int ch = g * Cg + c;
    const float sc = gamma[ch] * rs;
    scale[(long)n * C + ch] = sc;
    shift[(long)n * C + ch] = fmaf(-sc, mu, beta[ch]);
  }
}

// tok[n][s][c] = x[n][c][s] * scale[n][c] + shift[n][c]   (GroupNorm without activation, tokens-major for the Linear layers)
__global__ __launch_bounds__(256) void aekl_to_tokens_kernel(const float* __restrict__ x, const float* __restrict__ scale,
                                                             const float* __restrict__ shift, float* __restrict__ tok, int C,
                                                             int S) {
  __shared__ float tile[32][33];
  const int n = blockIdx.z, c0 = blockIdx.y * 32, s0 = blockIdx.x * 32;
  const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
  for (int r = ty; r < 32; r += 8) {
    const int c = c0 + r;
    const float v = x[((long)n * C + c) * S + s0 + tx];
    tile[r][tx] = scale ? fmaf(v, scale[(long)n * C + c], shift[(long)n * C + c]) : v;
  }
  __syncthreads();
  for (int r = ty; r < 32; r += 8) tok[((long)n * S + s0 + r) * C + c0 + tx] = tile[tx][r];
}

// y[n][c][s] = (tok[n][s][c] + res[n][c][s]) * mul
__global__ __launch_bounds__(256) void aekl_from_tokens_kernel(const float* __restrict__ tok, const float* __restrict__ res,
                                                               float* __restrict__ y, int C, int S, float mul) {
  __shared__ float tile[32][33];
  const int n = blockIdx.z, c0 = blockIdx.y * 32, s0 = blockIdx.x * 32;
  const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
  for (int r = ty; r < 32; r += 8) tile[r][tx] = tok[((long)n * S + s0 + r) * C + c0 + tx];
  __syncthreads();
  for (int r = ty; r < 32; r += 8) {
    const long o = ((long)n * C + c0 + r) * S + s0 + tx;
    float v = tile[tx][r];
    if (res) v += res[o];
    y[o] = v * mul;
  }
}

// y[row] = softmax(scale * x[row]); one workgroup per row, fixed reduction order
__global__ __launch_bounds__(256) void aekl_softmax_kernel(const float* __restrict__ x, float* __restrict__ y, int cols,
                                                           float scale) {
  __shared__ float smx[4];
  __shared__ double red[16];
  __shared__ double bc;
  const float* __restrict__ xr = x + (long)blockIdx.x * cols;
  float* __restrict__ yr = y + (long)blockIdx.x * cols;
  float mx = -INFINITY;
  for (int i = threadIdx.x; i < cols; i += 256) mx = fmaxf(mx, xr[i] * scale);
  mx = wave_max(mx);
  if ((threadIdx.x & 63) == 0) smx[threadIdx.x >> 6] = mx;
  __syncthreads();
  mx = fmaxf(fmaxf(smx[0], smx[1]), fmaxf(smx[2], smx[3]));
  float s = 0.f;
  for (int i = threadIdx.x; i < cols; i += 256) s += expf(xr[i] * scale - mx);
  const float inv = (float)(1.0 / block_sum_all((double)s, red, &bc));
  for (int i = threadIdx.x; i < cols; i += 256) yr[i] = expf(xr[i] * scale - mx) * inv;
}

__global__ __launch_bounds__(256) void aekl_posterior_kernel(const float* __restrict__ mom, const float* __restrict__ noise,
                                                             float* __restrict__ mean, float* __restrict__ logvar,
                                                             float* __restrict__ stdv, float* __restrict__ sample, long CHW,
                                                             long total) {
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= total) return;
  const long n = i / CHW, r = i - n * CHW;
  const float mu = mom[n * 2 * CHW + r];
  const float lv = fminf(fmaxf(mom[n * 2 * CHW + CHW + r], -30.0f), 20.0f);
  const float sd = expf(0.5f * lv);
  mean[i] = mu;
  logvar[i] = lv;
  stdv[i] = sd;
  if (sample) sample[i] = fmaf(sd, noise[i], mu);
}

// z (B, T, C, HW) of a frame sequence: frame f = b * T + t of the moments (B * T, 2C, HW) with the noise of draw t,
// noise (T, B, C, HW) — the sample of aekl_posterior_kernel, expression and order, and nothing else written.  VEC = 4:
// one 16-byte access per operand (CHW a multiple of 4, so a group of four never crosses a frame); VEC = 1: scalar.
template <int VEC>
__global__ __launch_bounds__(256) void aekl_posterior_seq_kernel(const float* __restrict__ mom, const float* __restrict__ noise,
                                                                 float* __restrict__ z, int B, int T, long CHW, long total) {
  const long stride = (long)gridDim.x * blockDim.x * VEC;
  for (long i = ((long)blockIdx.x * blockDim.x + threadIdx.x) * VEC; i < total; i += stride) {
    const long f = i / CHW, r = i - f * CHW;
    const long b = f / T, t = f - b * T;
    const float* pm = mom + f * 2 * CHW + r;
    const float* pn = noise + (t * B + b) * CHW + r;
    if constexpr (VEC == 4) {
      const float4 mu = *reinterpret_cast<const float4*>(pm);
      const float4 lr = *reinterpret_cast<const float4*>(pm + CHW);
      const float4 nz = *reinterpret_cast<const float4*>(pn);
      float4 o;
      o.x = fmaf(expf(0.5f * fminf(fmaxf(lr.x, -30.0f), 20.0f)), nz.x, mu.x);
      o.y = fmaf(expf(0.5f * fminf(fmaxf(lr.y, -30.0f), 20.0f)), nz.y, mu.y);
      o.z = fmaf(expf(0.5f * fminf(fmaxf(lr.z, -30.0f), 20.0f)), nz.z, mu.z);
      o.w = fmaf(expf(0.5f * fminf(fmaxf(lr.w, -30.0f), 20.0f)), nz.w, mu.w);
      *reinterpret_cast<float4*>(z + i) = o;
    } else {
      const float lv = fminf(fmaxf(pm[CHW], -30.0f), 20.0f);
      const float sd = expf(0.5f * lv);
      z[i] = fmaf(sd, *pn, *pm);
    }
  }
}

inline bool mode_ok(int mode) { return mode == MODE_BF16 || mode == MODE_SPLIT3 || mode == MODE_F32; }
inline int pad_to(int v, int m) { return (v + m - 1) / m * m; }

template <int KIND, int MODE>
int launch_conv3(const C3P& p, hipStream_t st) {
  constexpr size_t lds = (size_t)Geo<KIND>::PP * Rec<MODE>::B * (MODE == MODE_SPLIT3 ? 3 : 1);
  static_assert(lds <= kLdsLimit, "patch does not fit LDS");
  (void)hipFuncSetAttribute((const void*)aekl_conv3_kernel<KIND, MODE>, hipFuncAttributeMaxDynamicSharedMemorySize,
                            (int)kLdsLimit);
  const dim3 grid(cdiv(p.Wo, TW), cdiv(p.Ho, TH), p.N * p.ncb);
  hipLaunchKernelGGL((aekl_conv3_kernel<KIND, MODE>), grid, dim3(kThreads), lds, st, p);
  return check_launch("aekl_conv3_fwd");
}

template <int KIND>
int launch_conv3_mode(const C3P& p, int mode, hipStream_t st) {
  if (mode == MODE_BF16) return launch_conv3<KIND, MODE_BF16>(p, st);
  if (mode == MODE_SPLIT3) return launch_conv3<KIND, MODE_SPLIT3>(p, st);
  return launch_conv3<KIND, MODE_F32>(p, st);
}

}  // namespace

extern "C" {

size_t wfae_aekl_conv3_pack_bytes(int Cout, int Cin, int mode) {
  if (Cout <= 0 || Cin <= 0 || !mode_ok(mode)) return 0;
  const size_t elems = (size_t)pad_to(Cin, CK) / CK * 9 * pad_to(Cout, BM) * CK;
  return mode == MODE_F32 ? elems * 4 : elems * 2 * (size_t)mode;
}

int wfae_aekl_conv3_pack(const float* w, void* packed, int Cout, int Cin, int mode, wfae_stream_t stream) {
  WFAE_REQUIRE(w && packed, WFAE_ERR_NULL_POINTER, "aekl_conv3_pack: null pointer");
  WFAE_REQUIRE(mode_ok(mode), WFAE_ERR_BAD_SHAPE, "aekl_conv3_pack: mode %d (1 = bf16, 3 = three bf16 planes, 4 = fp32)", mode);
  WFAE_REQUIRE(Cout > 0 && Cin > 0 && Cout <= 4096 && Cin <= 4096, WFAE_ERR_UNSUPPORTED,
               "aekl_conv3_pack: channel counts 1..4096 are served (got Cout=%d Cin=%d)", Cout, Cin);
  WFAE_REQUIRE((reinterpret_cast<uintptr_t>(packed) & 15) == 0, WFAE_ERR_BAD_SHAPE, "aekl_conv3_pack: packed must be 16-byte aligned");
  const int CoutP = pad_to(Cout, BM), nchunks = pad_to(Cin, CK) / CK;
  const long total = (long)nchunks * 9 * CoutP * CK;
  const dim3 grid((unsigned)((total + 255) / 256));
  if (mode == MODE_F32)
    hipLaunchKernelGGL(aekl_pack_kernel<true>, grid, dim3(256), 0, (hipStream_t)stream, w, packed, Cout, Cin, CoutP, nchunks, 1);
  else
    hipLaunchKernelGGL(aekl_pack_kernel<false>, grid, dim3(256), 0, (hipStream_t)stream, w, packed, Cout, Cin, CoutP, nchunks, mode);
  return check_launch("aekl_conv3_pack");
}

int wfae_aekl_conv3_fwd(const float* x, const void* packed, const float* bias, const float* gn_scale, const float* gn_shift,
                        const float* res, float* y, int kind, int mode, int N, int Cin, int Cout, int H, int W,
                        float out_mul, wfae_stream_t stream) {
  WFAE_REQUIRE(x && packed && y, WFAE_ERR_NULL_POINTER, "aekl_conv3_fwd: null pointer");
  WFAE_REQUIRE((gn_scale == nullptr) == (gn_shift == nullptr), WFAE_ERR_NULL_POINTER,
               "aekl_conv3_fwd: the prologue needs both gn_scale and gn_shift");
  WFAE_REQUIRE(kind >= 0 && kind <= 2, WFAE_ERR_BAD_SHAPE,
               "aekl_conv3_fwd: kind %d (0 = stride 1, 1 = stride 2 with (0,1,0,1) padding, 2 = x2 nearest upsample + stride 1)", kind);
  WFAE_REQUIRE(mode_ok(mode), WFAE_ERR_BAD_SHAPE, "aekl_conv3_fwd: mode %d (1 = bf16, 3 = three bf16 planes, 4 = fp32)", mode);
  WFAE_REQUIRE(N > 0 && H > 0 && W > 0 && H <= 8192 && W <= 8192, WFAE_ERR_BAD_SHAPE, "aekl_conv3_fwd: bad shape N=%d H=%d W=%d",
               N, H, W);
  WFAE_REQUIRE(Cout > 0 && Cin > 0 && Cout <= 4096 && Cin <= 4096, WFAE_ERR_UNSUPPORTED,
               "aekl_conv3_fwd: channel counts 1..4096 are served (got Cout=%d Cin=%d)", Cout, Cin);
  WFAE_REQUIRE(kind != 1 || (H >= 2 && W >= 2), WFAE_ERR_BAD_SHAPE, "aekl_conv3_fwd: the stride-2 form needs a plane of at least 2x2");
  WFAE_REQUIRE((reinterpret_cast<uintptr_t>(packed) & 15) == 0, WFAE_ERR_BAD_SHAPE, "aekl_conv3_fwd: packed must be 16-byte aligned");
  C3P p = {};
  p.x = x; p.w = packed; p.bias = bias; p.gscale = gn_scale; p.gshift = gn_shift; p.res = res; p.y = y;
  p.N = N; p.Cin = Cin; p.Cout = Cout; p.H = H; p.W = W;
  p.CoutP = pad_to(Cout, BM);
  p.ncb = p.CoutP / BM;
  p.nchunks = pad_to(Cin, CK) / CK;
  p.Ho = kind == 0 ? H : kind == 1 ? (H - 2) / 2 + 1 : 2 * H;
  p.Wo = kind == 0 ? W : kind == 1 ? (W - 2) / 2 + 1 : 2 * W;
  p.out_mul = out_mul;
  WFAE_REQUIRE((long)Cin * H * W < (1l << 31) && (long)Cout * p.Ho * p.Wo < (1l << 31), WFAE_ERR_BAD_SHAPE,
               "aekl_conv3_fwd: one sample must stay below 2^31 elements");
  WFAE_REQUIRE((long)N * p.ncb <= 65535 && cdiv(p.Ho, TH) <= 65535, WFAE_ERR_BAD_SHAPE, "aekl_conv3_fwd: grid too large");
  hipStream_t st = (hipStream_t)stream;
  if (kind == 0) return launch_conv3_mode<0>(p, mode, st);
  if (kind == 1) return launch_conv3_mode<1>(p, mode, st);
  return launch_conv3_mode<2>(p, mode, st);
}

size_t wfae_aekl_gn_ws_bytes(int N, int C, int HW, int groups) {
  if (N <= 0 || C <= 0 || HW <= 0 || groups <= 0 || C % groups) return 0;
  const long L = (long)(C / groups) * HW;
  return (size_t)N * groups * cdiv(L, kGnSlice) * 2 * sizeof(double);
}

int wfae_aekl_gn_stats(const float* x, const float* gamma, const float* beta, float* mean, float* rstd, float* scale,
                       float* shift, int N, int C, int HW, int groups, float eps, void* ws, size_t ws_bytes,
                       wfae_stream_t stream) {
  WFAE_REQUIRE(x && gamma && beta && mean && rstd && scale && shift, WFAE_ERR_NULL_POINTER, "aekl_gn_stats: null pointer");
  WFAE_REQUIRE(N > 0 && C > 0 && HW > 0 && groups > 0 && C % groups == 0, WFAE_ERR_BAD_SHAPE,
               "aekl_gn_stats: bad shape N=%d C=%d HW=%d groups=%d", N, C, HW, groups);
  WFAE_REQUIRE((long)N * groups <= 65535, WFAE_ERR_BAD_SHAPE, "aekl_gn_stats: N * groups = %ld > 65535", (long)N * groups);
  const long L = (long)(C / groups) * HW;
  const int nblk = cdiv(L, kGnSlice);
  const size_t need = wfae_aekl_gn_ws_bytes(N, C, HW, groups);
  WFAE_REQUIRE(ws && ws_bytes >= need, WFAE_ERR_WORKSPACE, "aekl_gn_stats: workspace too small (%zu < %zu)", ws_bytes, need);
  WFAE_REQUIRE((reinterpret_cast<uintptr_t>(ws) & 7) == 0, WFAE_ERR_WORKSPACE, "aekl_gn_stats: workspace must be 8-byte aligned");
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(aekl_gn_part_kernel, dim3(nblk, N * groups), dim3(256), 0, st, x, (double*)ws, L, nblk);
  int rc = check_launch("aekl_gn_part");
  if (rc) return rc;
  hipLaunchKernelGGL(aekl_gn_final_kernel, dim3(N * groups), dim3(64), 0, st, (const double*)ws, gamma, beta, mean, rstd, scale,
                     shift, L, nblk, C, groups, eps);
  return check_launch("aekl_gn_final");
}

int wfae_aekl_to_tokens(const float* x, const float* scale, const float* shift, float* tok, int N, int C, int S,
                        wfae_stream_t stream) {
  WFAE_REQUIRE(x && tok, WFAE_ERR_NULL_POINTER, "aekl_to_tokens: null pointer");
  WFAE_REQUIRE((scale == nullptr) == (shift == nullptr), WFAE_ERR_NULL_POINTER, "aekl_to_tokens: scale and shift go together");
  WFAE_REQUIRE(N > 0 && N <= 65535 && C > 0 && S > 0, WFAE_ERR_BAD_SHAPE, "aekl_to_tokens: bad shape N=%d C=%d S=%d", N, C, S);
  WFAE_REQUIRE(C % 32 == 0 && S % 32 == 0 && C / 32 <= 65535, WFAE_ERR_UNSUPPORTED,
               "aekl_to_tokens: C and S must be multiples of 32 (got C=%d S=%d)", C, S);
  hipLaunchKernelGGL(aekl_to_tokens_kernel, dim3(S / 32, C / 32, N), dim3(256), 0, (hipStream_t)stream, x, scale, shift, tok, C, S);
  return check_launch("aekl_to_tokens");
}

int wfae_aekl_from_tokens(const float* tok, const float* res, float* y, int N, int C, int S, float mul, wfae_stream_t stream) {
  WFAE_REQUIRE(tok && y, WFAE_ERR_NULL_POINTER, "aekl_from_tokens: null pointer");
  WFAE_REQUIRE(N > 0 && N <= 65535 && C > 0 && S > 0, WFAE_ERR_BAD_SHAPE, "aekl_from_tokens: bad shape N=%d C=%d S=%d", N, C, S);
  WFAE_REQUIRE(C % 32 == 0 && S % 32 == 0 && C / 32 <= 65535, WFAE_ERR_UNSUPPORTED,
               "aekl_from_tokens: C and S must be multiples of 32 (got C=%d S=%d)", C, S);
  hipLaunchKernelGGL(aekl_from_tokens_kernel, dim3(S / 32, C / 32, N), dim3(256), 0, (hipStream_t)stream, tok, res, y, C, S, mul);
  return check_launch("aekl_from_tokens");
}

int wfae_aekl_softmax(const float* x, float* y, int64_t rows, int cols, float scale, wfae_stream_t stream) {
  WFAE_REQUIRE(x && y, WFAE_ERR_NULL_POINTER, "aekl_softmax: null pointer");
  WFAE_REQUIRE(rows > 0 && rows < (1ll << 31) && cols > 0, WFAE_ERR_BAD_SHAPE, "aekl_softmax: bad shape");
  hipLaunchKernelGGL(aekl_softmax_kernel, dim3((unsigned)rows), dim3(256), 0, (hipStream_t)stream, x, y, cols, scale);
  return check_launch("aekl_softmax");
}

int wfae_aekl_posterior(const float* moments, const float* noise, float* mean, float* logvar, float* std_, float* sample, int N,
                        int C, int HW, wfae_stream_t stream) {
  WFAE_REQUIRE(moments && mean && logvar && std_, WFAE_ERR_NULL_POINTER, "aekl_posterior: null pointer");
  WFAE_REQUIRE((noise == nullptr) == (sample == nullptr), WFAE_ERR_NULL_POINTER, "aekl_posterior: noise and sample go together");
  WFAE_REQUIRE(N > 0 && C > 0 && HW > 0, WFAE_ERR_BAD_SHAPE, "aekl_posterior: bad shape N=%d C=%d HW=%d", N, C, HW);
  const long CHW = (long)C * HW, total = CHW * N;
  WFAE_REQUIRE(total < (1l << 39), WFAE_ERR_BAD_SHAPE, "aekl_posterior: too large");
  hipLaunchKernelGGL(aekl_posterior_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream, moments, noise,
                     mean, logvar, std_, sample, CHW, total);
  return check_launch("aekl_posterior");
}

int wfae_aekl_posterior_seq(const float* moments, const float* noise, float* z, int B, int T, int C, int HW, wfae_stream_t stream) {
  WFAE_REQUIRE(moments && noise && z, WFAE_ERR_NULL_POINTER, "aekl_posterior_seq: null pointer");
  WFAE_REQUIRE(B > 0 && T > 0 && C > 0 && HW > 0, WFAE_ERR_BAD_SHAPE, "aekl_posterior_seq: bad shape B=%d T=%d C=%d HW=%d", B, T, C,
               HW);
  const long CHW = (long)C * HW, total = CHW * B * T;
  WFAE_REQUIRE(total < (1l << 39), WFAE_ERR_BAD_SHAPE, "aekl_posterior_seq: too large");
  const bool vec = HW % 4 == 0 && ((uintptr_t)moments | (uintptr_t)noise | (uintptr_t)z) % 16 == 0;
  const long items = vec ? total / 4 : total;
  const unsigned grid = (unsigned)((items + 255) / 256 < 2048 ? (items + 255) / 256 : 2048);     // 8 blocks per CU; grid-stride beyond
  if (vec)
    hipLaunchKernelGGL(aekl_posterior_seq_kernel<4>, dim3(grid), dim3(256), 0, (hipStream_t)stream, moments, noise, z, B, T, CHW, total);
  else
    hipLaunchKernelGGL(aekl_posterior_seq_kernel<1>, dim3(grid), dim3(256), 0, (hipStream_t)stream, moments, noise, z, B, T, CHW, total);
  return check_launch("aekl_posterior_seq");
}

}  // extern "C"
