// resae.hip — evaluation-mode forward kernels of the ae_gan residual autoencoders (reference
// experiments/v1_experiments/ae_gan/train.py `ResidualBlock`, `UpsampleBlock`, `ConvAutoencoder`, `ConvAutoencoderBIG`).
//
// One unit serves every layer of the blocks once BatchNorm is folded to its running statistics:
//     y = act( conv(x, w) * scale[co] + shift[co] + res )
// scale / shift: the folded BatchNorm (or a plain bias as shift alone), either may be null.  res: none, at the output's
// resolution, or read through a x2 nearest upsample (res[n, co, oy >> 1, ox >> 1]).  act: none or the exact GELU.
// kind 0: 3x3 stride 1 pad 1.  kind 1: 3x3 stride 2 pad 1 (Ho = (H - 1) / 2 + 1, input row 2 oy - 1 + ky).  kind 2: 3x3
// stride 1 pad 1 over the x2 nearest upsample of x (never written).  kind 3 / 4: the 1x1 shortcut with stride 1 / 2, which
// is the CENTRE tap of kind 0 / 1 (input row S oy): one geometry rule, input row = S oy + ky - 1, serves all five.
// NCHW fp32 in and out, fp32 accumulation, fixed summation order, no atomics: two launches give the same bits.
//
// Route 0, "tile": the implicit GEMM of aekl.hip's conv3 kernel (64 output channels x an 8 x 16 pixel tile of one sample
//   per workgroup, the LDS patch staged once per 32-channel chunk for all taps, weights packed [chunk][tap][co][32 ci],
//   modes 1 / 3 / 4 = bf16 / three bf16 planes / fp32 MFMA) with the stride-2 pad-1 and one-tap patches and the epilogue
//   above.  Serves every shape.
// Route 1, "small": layers whose output plane has at most 16 pixels are a weight stream.  The GEMM's columns are the
//   output pixels of ALL samples (n, oy, ox); a workgroup owns 64 output channels (16 per wave) x a group of 64 columns x
//   a share of the input-channel chunks, and reads its weights from HBM once: fp32, packed in the fragment order of
//   v_mfma_f32_16x16x4_f32 ([tap][16 co][16 ci] blocks of 64 lanes x 4 floats, a wave's load is 1 KiB contiguous).  The
//   input pixels of the group's samples are gathered into LDS per chunk; a tap is a per-lane offset into them, or a literal
//   zero where it is padding for that column.  DEAD taps (no output position of the layer reads a real pixel through
//   them: wfae_resae_live_taps) are neither fetched nor multiplied.  Where the K dimension is split over workgroups the
//   partial sums go to the workspace and are finished in ascending split order.
#include "common.h"
#include "resae_common.h"

using namespace wfae;
using namespace wfae::resae_geo;

namespace {

typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef unsigned u32x4 __attribute__((ext_vector_type(4)));

constexpr int BM = 64;            // output channels of a workgroup (both routes)
constexpr int TH = 8, TW = 16;    // output pixel tile of the tile route
constexpr int CK = 32;            // input channels per chunk (both routes)
constexpr int kThreads = 256;
constexpr size_t kLdsLimit = 160 * 1024;
constexpr int SCG = 64;           // columns of a column group of the small route
constexpr int SREC = CK + 4;      // floats of one LDS pixel record of the small route (padding spreads the banks)
constexpr int kSmallMaxPlane = 16;
constexpr int kSmallTargetWgs = 512;

enum { MODE_BF16 = 1, MODE_SPLIT3 = 3, MODE_F32 = 4 };

struct EP {
  const float* scale;
  const float* shift;
  const float* res;
  float* y;
  int Cout, Ho, Wo, res_mode, act;
};

__device__ __forceinline__ void ep_store(const EP& e, float v, int n, int co, int oy, int ox) {
  if (e.scale) v *= e.scale[co];
  if (e.shift) v += e.shift[co];
  const long o = (((long)n * e.Cout + co) * e.Ho + oy) * e.Wo + ox;
  if (e.res_mode == 1) v += e.res[o];
  else if (e.res_mode == 2) v += e.res[(((long)n * e.Cout + co) * (e.Ho >> 1) + (oy >> 1)) * (e.Wo >> 1) + (ox >> 1)];
  e.y[o] = e.act ? gelu_f(v) : v;
}

// ------------------------------------------------------------------------------------------------------- tile route
struct TP {
  const float* x;
  const void* w;
  EP e;
  int N, Cin, CoutP, H, W, nchunks, ncb;
};

template <int KIND>
struct Geo {
  static constexpr int T = KIND >= K1S1 ? 1 : 9;
  static constexpr int S = (KIND == K3S2 || KIND == K1S2) ? 2 : 1;
  static constexpr int PH = T == 1 ? TH : S * (TH - 1) + 3, PW = T == 1 ? TW : S * (TW - 1) + 3, PP = PH * PW;
};
template <int MODE>
struct Rec {
  static constexpr int B = MODE == MODE_F32 ? 144 : 80;
};

template <int KIND, int MODE>
__global__ __launch_bounds__(kThreads) void resae_tile_kernel(TP p) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  constexpr bool F32 = MODE == MODE_F32;
  constexpr int NP = F32 ? 1 : MODE;
  constexpr int T = Geo<KIND>::T, S = Geo<KIND>::S, PW = Geo<KIND>::PW, PP = Geo<KIND>::PP;
  constexpr int REC = Rec<MODE>::B;
  constexpr int PLANE = PP * REC;
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6, r15 = lane & 15, g4 = lane >> 4;
  const int ox0 = blockIdx.x * TW, oy0 = blockIdx.y * TH;
  const int n = blockIdx.z / p.ncb, co0 = (blockIdx.z % p.ncb) * BM;
  const int HW = p.H * p.W;
  const float* __restrict__ xn = p.x + (long)n * p.Cin * HW;
  const long wplane = (long)p.nchunks * T * p.CoutP * CK;   // elements of one packed plane

  f32x4 acc[4][2];
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
      for (int q = 0; q < 4; ++q) acc[i][j][q] = 0.f;

  for (int cc = 0; cc < p.nchunks; ++cc) {
    // two-level summation as in aekl.hip: the MFMAs of a chunk accumulate from zero, the chunk sums are added up
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
      if (T == 1) {
        sy = S * (oy0 + py); sx = S * (ox0 + px);
        ok = sy < p.H && sx < p.W;
      } else if (KIND == K3UP) {
        const int uy = oy0 - 1 + py, ux = ox0 - 1 + px;
        ok = uy >= 0 && uy < 2 * p.H && ux >= 0 && ux < 2 * p.W;
        sy = uy >> 1; sx = ux >> 1;
      } else {
        sy = S * oy0 - 1 + py; sx = S * ox0 - 1 + px;
        ok = sy >= 0 && sy < p.H && sx >= 0 && sx < p.W;
      }
      const int c0 = cc * CK + g * 8;
      float v[8];
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const int ci = c0 + j;
        v[j] = (ok && ci < p.Cin) ? xn[(long)ci * HW + sy * p.W + sx] : 0.f;   // padding pixels and channels: zeros
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

    // ---- the taps: shifted fragment reads of the same patch
#pragma unroll
    for (int tap = 0; tap < T; ++tap) {
      const int ky = tap / 3, kx = tap % 3;
      const long wrow = ((long)(cc * T + tap) * p.CoutP + co0 + r15) * CK;   // + 16 i * CK
      int pixj[2];
#pragma unroll
      for (int j = 0; j < 2; ++j)
        pixj[j] = T == 1 ? (2 * wave + j) * PW + r15 : (S * (2 * wave + j) + ky) * PW + S * r15 + kx;
      if constexpr (!F32) {
        const unsigned short* __restrict__ wp = reinterpret_cast<const unsigned short*>(p.w);
        bf16x8 a[4][NP], b[2][NP];
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
          for (int pl = 0; pl < NP; ++pl)
            a[i][pl] = *reinterpret_cast<const bf16x8*>(wp + pl * wplane + wrow + 16 * i * CK + 8 * g4);
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
          for (int pl = 0; pl < NP; ++pl)
            b[j][pl] = *reinterpret_cast<const bf16x8*>(smem + pl * PLANE + pixj[j] * REC + 16 * g4);
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
          for (int j = 0; j < 2; ++j) b[j] = *reinterpret_cast<const f32x4*>(smem + pixj[j] * REC + 64 * hf + 16 * g4);
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
    if (oy >= p.e.Ho || ox >= p.e.Wo) continue;
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const int co = co0 + 16 * i + 4 * g4 + q;
        if (co < p.e.Cout) ep_store(p.e, acc[i][j][q], n, co, oy, ox);
      }
  }
}

// packed[plane][chunk][tap][co < CoutP][32 ci] (aekl.hip's layout with T taps); zeros in the channel padding
template <bool F32>
__global__ __launch_bounds__(256) void resae_pack_tile_kernel(const float* __restrict__ w, void* __restrict__ out, int Cout, int Cin,
                                                              int CoutP, int nchunks, int T, int planes) {
  const long total = (long)nchunks * T * CoutP * CK;
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= total) return;
  const int k = (int)(i % CK);
  const long r = i / CK;
  const int co = (int)(r % CoutP);
  const int ct = (int)(r / CoutP), tap = ct % T, cc = ct / T;
  const int ci = cc * CK + k;
  const float v = (co < Cout && ci < Cin) ? w[((long)co * Cin + ci) * T + tap] : 0.f;
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

// ------------------------------------------------------------------------------------------------------ small route
struct SP {
  const float* x;
  const float* w;
  float* ws;
  EP e;
  int kind, N, Cin, H, W, R, ncob, nkb, nchunks, per_split, splits, live;
};

// packed[tap < T][cob][kb][lane = 16 g4 + r15][c < 4] = w[co = 16 cob + r15][ci = 16 kb + 4 g4 + c][tap]
__global__ __launch_bounds__(256) void resae_pack_small_kernel(const float* __restrict__ w, float* __restrict__ out, int Cout, int Cin,
                                                               int ncob, int nkb, int T) {
  const long total = (long)T * ncob * nkb * 256;
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= total) return;
  const int c = (int)(i & 3), lane = (int)((i >> 2) & 63);
  long r = i >> 8;
  const int kb = (int)(r % nkb);
  r /= nkb;
  const int cob = (int)(r % ncob), tap = (int)(r / ncob);
  const int co = 16 * cob + (lane & 15), ci = 16 * kb + 4 * (lane >> 4) + c;
  out[i] = (co < Cout && ci < Cin) ? w[((long)co * Cin + ci) * T + tap] : 0.f;
}

__global__ __launch_bounds__(kThreads) void resae_small_kernel(SP p) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  float* xs = reinterpret_cast<float*>(smem);
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6, r15 = lane & 15, g4 = lane >> 4;
  const int cob = blockIdx.x * 4 + wave;
  const bool wave_on = cob < p.ncob;
  const int col0 = blockIdx.y * SCG;
  const int T = kind_taps(p.kind);
  const int HW = p.H * p.W, HoWo = p.e.Ho * p.e.Wo;
  const int n0 = col0 / HoWo;
  const int n1 = min(p.N - 1, (col0 + SCG - 1) / HoWo);
  const int npix = (n1 - n0 + 1) * HW;
  const int cc0 = blockIdx.z * p.per_split, cc1 = min(p.nchunks, cc0 + p.per_split);

  // this lane's four columns (one per 16-column tile) and, per tap, the LDS record they read or -1 for a literal zero
  int cn[4], coy[4], cox[4], off[4][9];
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int col = col0 + 16 * j + r15;
    const bool cv = col < p.R;
    const int n = cv ? col / HoWo : n0, o = cv ? col % HoWo : 0;
    cn[j] = cv ? n : -1;
    coy[j] = o / p.e.Wo;
    cox[j] = o % p.e.Wo;
#pragma unroll
    for (int tap = 0; tap < 9; ++tap) {
      const int sy = src_index(p.kind, coy[j], tap / 3, p.H), sx = src_index(p.kind, cox[j], tap % 3, p.W);
      off[j][tap] = (cv && sy >= 0 && sx >= 0) ? ((n - n0) * HW + sy * p.W + sx) * SREC : -1;
    }
  }

  f32x4 acc[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) acc[j] = f32x4{0.f, 0.f, 0.f, 0.f};

  for (int cc = cc0; cc < cc1; ++cc) {
    // the chunk's weights first: their HBM latency runs under the staging of the columns
    f32x4 a[9][2];
#pragma unroll
    for (int tap = 0; tap < 9; ++tap)
#pragma unroll
      for (int hf = 0; hf < 2; ++hf) {
        a[tap][hf] = f32x4{0.f, 0.f, 0.f, 0.f};
        if (wave_on && ((p.live >> tap) & 1)) {
          const int ts = T == 9 ? tap : 0;
          a[tap][hf] = *reinterpret_cast<const f32x4*>(p.w + ((((long)ts * p.ncob + cob) * p.nkb + 2 * cc + hf) * 64 + lane) * 4);
        }
      }
    __syncthreads();   // the fragment reads of the previous chunk are done
    // ---- gather the input pixels of samples n0..n1: item = (pixel, group of 4 channels); lanes run along the pixels
    for (int it = t; it < npix * 8; it += kThreads) {
      const int pix = it % npix, g = it / npix;
      const int nr = pix / HW, ip = pix - nr * HW;
      const float* __restrict__ xp = p.x + ((long)(n0 + nr) * p.Cin) * HW + ip;
      const int c0 = cc * CK + 4 * g;
      f32x4 v;
#pragma unroll
      for (int j = 0; j < 4; ++j) v[j] = (c0 + j < p.Cin) ? xp[(long)(c0 + j) * HW] : 0.f;
      *reinterpret_cast<f32x4*>(xs + pix * SREC + 4 * g) = v;
    }
    __syncthreads();
    if (wave_on) {
      f32x4 part[4];   // two-level summation: the chunk accumulates from zero
#pragma unroll
      for (int j = 0; j < 4; ++j) part[j] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int tap = 0; tap < 9; ++tap) {
        if (!((p.live >> tap) & 1)) continue;   // dead taps: not fetched, not multiplied
#pragma unroll
        for (int hf = 0; hf < 2; ++hf) {
          f32x4 b[4];
#pragma unroll
          for (int j = 0; j < 4; ++j) {
            b[j] = f32x4{0.f, 0.f, 0.f, 0.f};
            if (off[j][tap] >= 0) b[j] = *reinterpret_cast<const f32x4*>(xs + off[j][tap] + 16 * hf + 4 * g4);
          }
#pragma unroll
          for (int c = 0; c < 4; ++c)
#pragma unroll
            for (int j = 0; j < 4; ++j) part[j] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[tap][hf][c], b[j][c], part[j], 0, 0, 0);
        }
      }
#pragma unroll
      for (int j = 0; j < 4; ++j) acc[j] += part[j];
    }
  }
  if (!wave_on) return;
  // accumulator register q of lane (r15, g4) is (co = 16 cob + 4 g4 + q, column 16 j + r15 of the group)
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    if (cn[j] < 0) continue;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int co = 16 * cob + 4 * g4 + q;
      if (p.splits == 1) {
        if (co < p.e.Cout) ep_store(p.e, acc[j][q], cn[j], co, coy[j], cox[j]);
      } else {
        p.ws[((long)blockIdx.z * p.ncob * 16 + co) * p.R + col0 + 16 * j + r15] = acc[j][q];
      }
    }
  }
}

// the partial sums of the K splits, added in ascending split order, then the epilogue
__global__ __launch_bounds__(256) void resae_small_final_kernel(const float* __restrict__ ws, EP e, int R, int rows, int splits) {
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= (long)e.Cout * R) return;
  const int co = (int)(i / R), col = (int)(i % R);
  float v = 0.f;
  for (int s = 0; s < splits; ++s) v += ws[((long)s * rows + co) * R + col];
  const int HoWo = e.Ho * e.Wo, o = col % HoWo;
  ep_store(e, v, col / HoWo, co, o / e.Wo, o % e.Wo);
}

struct Plan {
  int ncob, nkb, nchunks, slabs, cgs, splits, per_split, R;
  size_t ws, lds;
};

Plan plan_small(int kind, int N, int Cin, int Cout, int H, int W) {
  Plan q = {};
  const int Ho = out_size(kind, H), Wo = out_size(kind, W), HoWo = Ho * Wo;
  q.ncob = cdiv(Cout, 16);
  q.nchunks = cdiv(Cin, CK);
  q.nkb = 2 * q.nchunks;
  q.slabs = cdiv(q.ncob, 4);
  q.R = N * HoWo;
  q.cgs = cdiv(q.R, SCG);
  int splits = cdiv(kSmallTargetWgs, (int64_t)q.slabs * q.cgs);
  splits = splits < 1 ? 1 : splits > q.nchunks ? q.nchunks : splits;
  q.per_split = cdiv(q.nchunks, splits);
  q.splits = cdiv(q.nchunks, q.per_split);
  q.ws = q.splits > 1 ? (size_t)q.splits * q.ncob * 16 * q.R * sizeof(float) : 0;
  const int cap = (SCG - 1) / HoWo + 2, ns = N < cap ? N : cap;   // samples a column group can touch
  q.lds = (size_t)ns * H * W * SREC * sizeof(float);
  return q;
}

inline bool mode_ok(int mode) { return mode == MODE_BF16 || mode == MODE_SPLIT3 || mode == MODE_F32; }
inline int pad_to(int v, int m) { return (v + m - 1) / m * m; }

int check_layer(const char* what, int route, int kind, int mode, int Cout, int Cin) {
  WFAE_REQUIRE(route == 0 || route == 1, WFAE_ERR_BAD_SHAPE, "%s: route %d (0 = tile, 1 = small)", what, route);
  WFAE_REQUIRE(kind >= K3S1 && kind <= K1S2, WFAE_ERR_BAD_SHAPE,
               "%s: kind %d (0 = 3x3 s1 p1, 1 = 3x3 s2 p1, 2 = x2 nearest upsample + 3x3 s1 p1, 3 = 1x1 s1, 4 = 1x1 s2)", what, kind);
  WFAE_REQUIRE(route == 1 || mode_ok(mode), WFAE_ERR_BAD_SHAPE, "%s: mode %d (1 = bf16, 3 = three bf16 planes, 4 = fp32)", what, mode);
  WFAE_REQUIRE(Cout > 0 && Cin > 0 && Cout <= 4096 && Cin <= 4096, WFAE_ERR_UNSUPPORTED,
               "%s: channel counts 1..4096 are served (got Cout=%d Cin=%d)", what, Cout, Cin);
  return WFAE_OK;
}

size_t pack_bytes(int route, int kind, int mode, int Cout, int Cin) {
  const size_t T = kind_taps(kind);
  if (route == 1) return T * cdiv(Cout, 16) * 2 * cdiv(Cin, CK) * 256 * sizeof(float);
  const size_t elems = (size_t)cdiv(Cin, CK) * T * pad_to(Cout, BM) * CK;
  return mode == MODE_F32 ? elems * 4 : elems * 2 * (size_t)mode;
}

template <int KIND, int MODE>
int launch_tile(const TP& p, hipStream_t st) {
  constexpr size_t lds = (size_t)Geo<KIND>::PP * Rec<MODE>::B * (MODE == MODE_SPLIT3 ? 3 : 1);
  static_assert(lds <= kLdsLimit, "patch does not fit LDS");
  (void)hipFuncSetAttribute((const void*)resae_tile_kernel<KIND, MODE>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)kLdsLimit);
  const dim3 grid(cdiv(p.e.Wo, TW), cdiv(p.e.Ho, TH), p.N * p.ncb);
  hipLaunchKernelGGL((resae_tile_kernel<KIND, MODE>), grid, dim3(kThreads), lds, st, p);
  return check_launch("resae_conv (tile)");
}

template <int KIND>
int launch_tile_mode(const TP& p, int mode, hipStream_t st) {
  if (mode == MODE_BF16) return launch_tile<KIND, MODE_BF16>(p, st);
  if (mode == MODE_SPLIT3) return launch_tile<KIND, MODE_SPLIT3>(p, st);
  return launch_tile<KIND, MODE_F32>(p, st);
}

}  // namespace

extern "C" {

int wfae_resae_live_taps(int kind, int H, int W) {
  WFAE_REQUIRE(kind >= K3S1 && kind <= K1S2, WFAE_ERR_BAD_SHAPE, "resae_live_taps: kind %d, expected 0..4", kind);
  WFAE_REQUIRE(H > 0 && W > 0 && H <= 8192 && W <= 8192, WFAE_ERR_BAD_SHAPE, "resae_live_taps: bad plane %dx%d", H, W);
  return live_mask(kind, H, W);
}

size_t wfae_resae_pack_bytes(int route, int kind, int mode, int Cout, int Cin) {
  if (check_layer("resae_pack_bytes", route, kind, mode, Cout, Cin)) return 0;
  return pack_bytes(route, kind, mode, Cout, Cin);
}

int wfae_resae_pack(const float* w, void* packed, int route, int kind, int mode, int Cout, int Cin, wfae_stream_t stream) {
  WFAE_REQUIRE(w && packed, WFAE_ERR_NULL_POINTER, "resae_pack: null pointer");
  int rc = check_layer("resae_pack", route, kind, mode, Cout, Cin);
  if (rc) return rc;
  WFAE_REQUIRE((reinterpret_cast<uintptr_t>(packed) & 15) == 0, WFAE_ERR_BAD_SHAPE, "resae_pack: packed must be 16-byte aligned");
  const int T = kind_taps(kind);
  hipStream_t st = (hipStream_t)stream;
  if (route == 1) {
    const int ncob = cdiv(Cout, 16), nkb = 2 * cdiv(Cin, CK);
    const long total = (long)T * ncob * nkb * 256;
    hipLaunchKernelGGL(resae_pack_small_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st, w, (float*)packed, Cout, Cin,
                       ncob, nkb, T);
    return check_launch("resae_pack");
  }
  const int CoutP = pad_to(Cout, BM), nchunks = cdiv(Cin, CK);
  const long total = (long)nchunks * T * CoutP * CK;
  const dim3 grid((unsigned)((total + 255) / 256));
  if (mode == MODE_F32)
    hipLaunchKernelGGL(resae_pack_tile_kernel<true>, grid, dim3(256), 0, st, w, packed, Cout, Cin, CoutP, nchunks, T, 1);
  else
    hipLaunchKernelGGL(resae_pack_tile_kernel<false>, grid, dim3(256), 0, st, w, packed, Cout, Cin, CoutP, nchunks, T, mode);
  return check_launch("resae_pack");
}

size_t wfae_resae_workspace_bytes(int kind, int N, int Cin, int Cout, int H, int W) {
  if (kind < K3S1 || kind > K1S2 || N <= 0 || Cin <= 0 || Cout <= 0 || H <= 0 || W <= 0 || Cin > 4096 || Cout > 4096) return 0;
  if ((long)out_size(kind, H) * out_size(kind, W) > kSmallMaxPlane || (long)N * out_size(kind, H) * out_size(kind, W) >= (1l << 21)) return 0;
  return plan_small(kind, N, Cin, Cout, H, W).ws;
}

int wfae_resae_conv(const float* x, const void* packed, const float* scale, const float* shift, const float* res, float* y,
                    int route, int kind, int mode, int res_mode, int act, int N, int Cin, int Cout, int H, int W, void* ws,
                    size_t ws_bytes, wfae_stream_t stream) {
  WFAE_REQUIRE(x && packed && y, WFAE_ERR_NULL_POINTER, "resae_conv: null pointer");
  int rc = check_layer("resae_conv", route, kind, mode, Cout, Cin);
  if (rc) return rc;
  WFAE_REQUIRE(res_mode >= 0 && res_mode <= 2 && (res != nullptr) == (res_mode != 0), WFAE_ERR_BAD_SHAPE,
               "resae_conv: res_mode %d (0 = none, 1 = at the output's resolution, 2 = through a x2 nearest upsample) goes with res "
               "exactly when it is not 0", res_mode);
  WFAE_REQUIRE(act == 0 || act == 1, WFAE_ERR_BAD_SHAPE, "resae_conv: act %d (0 = none, 1 = GELU)", act);
  WFAE_REQUIRE(N > 0 && H > 0 && W > 0 && H <= 8192 && W <= 8192, WFAE_ERR_BAD_SHAPE, "resae_conv: bad shape N=%d H=%d W=%d", N, H, W);
  WFAE_REQUIRE((reinterpret_cast<uintptr_t>(packed) & 15) == 0, WFAE_ERR_BAD_SHAPE, "resae_conv: packed must be 16-byte aligned");
  const int Ho = out_size(kind, H), Wo = out_size(kind, W);
  WFAE_REQUIRE(res_mode != 2 || (Ho % 2 == 0 && Wo % 2 == 0), WFAE_ERR_BAD_SHAPE,
               "resae_conv: a residual read through the upsample needs an even output plane (got %dx%d)", Ho, Wo);
  WFAE_REQUIRE((long)Cin * H * W < (1l << 31) && (long)Cout * Ho * Wo < (1l << 31), WFAE_ERR_BAD_SHAPE,
               "resae_conv: one sample must stay below 2^31 elements");
  EP e = {scale, shift, res, y, Cout, Ho, Wo, res_mode, act};
  hipStream_t st = (hipStream_t)stream;
  if (route == 1) {
    WFAE_REQUIRE((long)Ho * Wo <= kSmallMaxPlane, WFAE_ERR_UNSUPPORTED,
                 "resae_conv: the small-plane route serves output planes of at most %d pixels (got %dx%d)", kSmallMaxPlane, Ho, Wo);
    WFAE_REQUIRE((long)N * Ho * Wo < (1l << 21), WFAE_ERR_UNSUPPORTED, "resae_conv: the small-plane route serves N Ho Wo < 2^21");
    const Plan q = plan_small(kind, N, Cin, Cout, H, W);
    WFAE_REQUIRE(q.lds <= 64 * 1024, WFAE_ERR_UNSUPPORTED, "resae_conv: the small-plane route needs %zu bytes of LDS for a %dx%d input",
                 q.lds, H, W);
    WFAE_REQUIRE(q.ws == 0 || (ws && ws_bytes >= q.ws), WFAE_ERR_WORKSPACE, "resae_conv: workspace too small (%zu < %zu)", ws_bytes, q.ws);
    WFAE_REQUIRE(q.ws == 0 || (reinterpret_cast<uintptr_t>(ws) & 3) == 0, WFAE_ERR_WORKSPACE, "resae_conv: workspace must be 4-byte aligned");
    SP p = {};
    p.x = x; p.w = (const float*)packed; p.ws = (float*)ws; p.e = e;
    p.kind = kind; p.N = N; p.Cin = Cin; p.H = H; p.W = W; p.R = q.R; p.ncob = q.ncob; p.nkb = q.nkb; p.nchunks = q.nchunks;
    p.per_split = q.per_split; p.splits = q.splits; p.live = live_mask(kind, H, W);
    (void)hipFuncSetAttribute((const void*)resae_small_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, 64 * 1024);
    hipLaunchKernelGGL(resae_small_kernel, dim3(q.slabs, q.cgs, q.splits), dim3(kThreads), q.lds, st, p);
    if ((rc = check_launch("resae_conv (small)"))) return rc;
    if (q.splits > 1) {
      // one thread per output element (Cout * R <= 2^12 * 2^21: at most 2^25 workgroups); not a grid-stride kernel
      hipLaunchKernelGGL(resae_small_final_kernel, dim3((unsigned)(((long)Cout * q.R + 255) / 256)), dim3(256), 0, st,
                         (const float*)ws, e, q.R, q.ncob * 16, q.splits);
      rc = check_launch("resae_conv (small, final)");
    }
    return rc;
  }
  TP p = {};
  p.x = x; p.w = packed; p.e = e;
  p.N = N; p.Cin = Cin; p.H = H; p.W = W;
  p.CoutP = pad_to(Cout, BM);
  p.ncb = p.CoutP / BM;
  p.nchunks = cdiv(Cin, CK);
  WFAE_REQUIRE((long)N * p.ncb <= 65535 && cdiv(Ho, TH) <= 65535, WFAE_ERR_BAD_SHAPE, "resae_conv: grid too large");
  switch (kind) {
    case K3S1: return launch_tile_mode<K3S1>(p, mode, st);
    case K3S2: return launch_tile_mode<K3S2>(p, mode, st);
    case K3UP: return launch_tile_mode<K3UP>(p, mode, st);
    case K1S1: return launch_tile_mode<K1S1>(p, mode, st);
    default: return launch_tile_mode<K1S2>(p, mode, st);
  }
}

}  // extern "C"
