// aekl_bwd.hip — backward kernels of the AutoencoderKL (forward: aekl.hip).  NCHW fp32 in and out, fixed summation order,
// no atomics: two launches give the same bits.
//
// conv3_bwd_data: du = conv(dy, w rotated 180 degrees, in / out transposed) * silu'(x * scale + shift) — the gradient of the
//   forward prologue's PRE-activation u (null scale / shift: no factor).  The tile loop is aekl_conv3_kernel's (64 channels x
//   an 8 x 16 pixel tile per workgroup, the patch of a 32-channel chunk staged once for nine taps, the packed weights of
//   wfae_aekl_conv3_pack applied to w.flip(2, 3).transpose(0, 1), the same three operand modes, two-level summation); what
//   differs per kind is the loader and the epilogue:
//   kind 0: dy read with pad 1.
//   kind 1 (the forward's stride 2 over the (0, 1, 0, 1)-padded input): dy is read through zero insertion — patch pixel
//     (zy, zx) of the plane of x holds dy[zy / 2, zx / 2] where both are even and inside Ho x Wo, else zero, with two
//     pixels of padding in front:  dx[y, x] = sum_k dy[(y - ky) / 2, (x - kx) / 2] w[ky, kx].
//   kind 2 (the forward's conv over the nearest x2 upsample): kind 0 on the 2H x 2W grid, and the epilogue adds up each
//     2 x 2 block in registers (the two tile rows of a wave, then the neighbouring lane) — the 4x tensor is never written.
// conv3_bwd_weight: dW[co, ci, ky, kx] = sum_{n, oy, ox} dy[n, co, oy, ox] a[n, ci, .],  a = SiLU(x * scale + shift)
//   recomputed on load (padding taps literal zeros AFTER it), on v_mfma_f32_16x16x32_bf16 with the PIXELS as the K dimension.
//   A workgroup of 4 waves owns 64 co x 32 ci x 9 taps; wave w owns co rows 16 w .. 16 w + 15: 2 x 9 accumulator tiles, 72
//   fp32 per lane.  Per pixel tile (8 x 16; 4 x 16 for kind 1) it stages in LDS, as bf16 planes with the pixels contiguous,
//   the dy tile [64 co][tile pixels] and ONE patch of a [32 ci][patch rows][patch columns] for all nine taps.  An MFMA's K
//   step is 32 pixels = 2 tile rows (4 lane groups x 8 consecutive columns).  A tap is a shifted read of the patch: ky
//   moves the row; kx moves the column by 0..2 bf16 elements, which a 16-byte LDS read cannot address, so a lane reads the
//   two aligned 16-byte pieces around its 8 columns once per (ky, ci fragment, plane) and funnels the three kx fragments
//   out of them in registers.  Kind 1 reads columns 2 ox + kx: the patch is staged de-interleaved by column parity, so
//   kx = 0 / 1 / 2 is (even half, shift 0) / (odd half, shift 0) / (even half, shift 1).
//   The reduction over pixels is split across workgroups by sample and by groups of kWgTiles pixel tiles.  The MFMAs of a
//   tile accumulate from zero (24 in a chain in mode 3), the tile sums are added to the workgroup's accumulators, and
//   those go to a slab [9][Cout][Cin] of the workspace; the finalize kernel adds the slabs in ascending order (in fp64) and
//   writes dW in its (Cout, Cin, 3, 3) layout.  The levels are there for the reason given at the forward's chunk loop.
//   mode 3: both operands as three exact bf16 planes, six products per fp32 product.  mode 1: the h plane alone (the operand
//   rounded after the prologue).  mode 4 is not served.
// gn_bwd: GroupNorm backward from du (the gradient of u = gamma xhat + beta) and x: one statistics pass (per (sample,
//   channel) sum du and sum du xhat in fp64, xhat taken as (x - mean) rstd, no E[x^2] shortcuts), a finalize launch (per
//   (sample, group) s1 = sum_c gamma_c sum du, s2 = sum_c gamma_c sum du xhat; per channel dbeta, dgamma over the samples in
//   ascending order) and one apply pass  dx = rstd (du gamma_c - (s1 + xhat s2) / m) + skip.
// softmax_bwd, posterior_bwd: elementwise / per row.
#include "common.h"

using namespace wfae;

namespace {

typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef unsigned u32x4 __attribute__((ext_vector_type(4)));

constexpr int BM = 64;            // channels of a workgroup's output (dgrad: of du; wgrad: co)
constexpr int TH = 8, TW = 16;    // pixel tile of the data gradient
constexpr int CK = 32;            // channels per chunk (dgrad: of dy; wgrad: ci)
constexpr int kThreads = 256;
constexpr size_t kLdsLimit = 160 * 1024;

enum { MODE_BF16 = 1, MODE_SPLIT3 = 3, MODE_F32 = 4 };

__device__ __forceinline__ float silu_f(float v) { return v / (1.0f + expf(-v)); }
__device__ __forceinline__ float silu_grad_f(float u) {
  const float s = 1.0f / (1.0f + expf(-u));
  return s * fmaf(u, 1.0f - s, 1.0f);
}

#define WFAE_PK(a, j) ((unsigned)a[j] | ((unsigned)a[j + 1] << 16))

// ------------------------------------------------------------------------------------------------ data gradient
struct D3P {
  const float* dy;      // (N, Cd, Hd, Wd)
  const void* w;        // packed w.flip(2, 3).transpose(0, 1): (Cx, Cd, 3, 3)
  const float* x;       // (N, Cx, H, W), read only with the prologue factor
  const float* gscale;
  const float* gshift;
  float* du;            // (N, Cx, H, W)
  int N, Cd, Cx, CxP, Hd, Wd, H, W, nchunks, ncb;
};

constexpr int DPH = TH + 2, DPW = TW + 2, DPP = DPH * DPW;
template <int MODE>
struct Rec {
  static constexpr int B = MODE == MODE_F32 ? 144 : 80;   // aekl.hip Rec
};

template <int KIND, int MODE>
__global__ __launch_bounds__(kThreads) void aekl_dgrad_kernel(D3P p) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  constexpr bool F32 = MODE == MODE_F32;
  constexpr int NP = F32 ? 1 : MODE;
  constexpr int REC = Rec<MODE>::B;
  constexpr int PLANE = DPP * REC;
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6, r15 = lane & 15, g4 = lane >> 4;
  const int ox0 = blockIdx.x * TW, oy0 = blockIdx.y * TH;
  const int n = blockIdx.z / p.ncb, co0 = (blockIdx.z % p.ncb) * BM;
  const int HWd = p.Hd * p.Wd;
  const float* __restrict__ dyn = p.dy + (long)n * p.Cd * HWd;
  const long wplane = (long)p.nchunks * 9 * p.CxP * CK;

  f32x4 acc[4][2];
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
      for (int q = 0; q < 4; ++q) acc[i][j][q] = 0.f;

  for (int cc = 0; cc < p.nchunks; ++cc) {
    f32x4 part[4][2];   // two-level summation (aekl.hip)
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
      for (int j = 0; j < 2; ++j)
#pragma unroll
        for (int q = 0; q < 4; ++q) part[i][j][q] = 0.f;
    __syncthreads();
    for (int it = t; it < DPP * 4; it += kThreads) {
      const int pix = it % DPP, g = it / DPP;
      const int py = pix / DPW, px = pix - py * DPW;
      int sy, sx;
      bool ok;
      if (KIND == 1) {
        const int zy = oy0 - 2 + py, zx = ox0 - 2 + px;   // the zero-inserted plane, two pixels of padding in front
        sy = zy >> 1; sx = zx >> 1;
        ok = zy >= 0 && zx >= 0 && !(zy & 1) && !(zx & 1) && sy < p.Hd && sx < p.Wd;
      } else {
        sy = oy0 - 1 + py; sx = ox0 - 1 + px;
        ok = sy >= 0 && sy < p.Hd && sx >= 0 && sx < p.Wd;
      }
      const int c0 = cc * CK + g * 8;
      float v[8];
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const int ci = c0 + j;
        v[j] = (ok && ci < p.Cd) ? dyn[(long)ci * HWd + sy * p.Wd + sx] : 0.f;
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
        *reinterpret_cast<u32x4*>(dst) = u32x4{WFAE_PK(h, 0), WFAE_PK(h, 2), WFAE_PK(h, 4), WFAE_PK(h, 6)};
        *reinterpret_cast<u32x4*>(dst + PLANE) = u32x4{WFAE_PK(m, 0), WFAE_PK(m, 2), WFAE_PK(m, 4), WFAE_PK(m, 6)};
        *reinterpret_cast<u32x4*>(dst + 2 * PLANE) = u32x4{WFAE_PK(l, 0), WFAE_PK(l, 2), WFAE_PK(l, 4), WFAE_PK(l, 6)};
      }
    }
    __syncthreads();

#pragma unroll
    for (int tap = 0; tap < 9; ++tap) {
      const int ky = tap / 3, kx = tap % 3;
      const long wrow = ((long)(cc * 9 + tap) * p.CxP + co0 + r15) * CK;
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
          const int pix = (2 * wave + j + ky) * DPW + r15 + kx;
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
        const float* __restrict__ wp = reinterpret_cast<const float*>(p.w);
#pragma unroll
        for (int hf = 0; hf < 2; ++hf) {
          f32x4 a[4], b[2];
#pragma unroll
          for (int i = 0; i < 4; ++i) a[i] = *reinterpret_cast<const f32x4*>(wp + wrow + 16 * i * CK + 16 * hf + 4 * g4);
#pragma unroll
          for (int j = 0; j < 2; ++j) {
            const int pix = (2 * wave + j + ky) * DPW + r15 + kx;
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

  // ---- epilogue: accumulator register q of lane (r15, g4) is (channel 16 i + 4 g4 + q, pixel r15 of tile row 2 wave + j)
  const int HW = p.H * p.W;
  const bool pro = p.gscale != nullptr;
  if (KIND == 2) {
    // the 2 x 2 block sum: rows 2 wave and 2 wave + 1 are one source row, lanes r15 and r15 ^ 1 one source column
    const int sy = (oy0 >> 1) + wave, sx = (ox0 + r15) >> 1;
    const bool mine = !(r15 & 1) && sy < p.H && sx < p.W;
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        float v = acc[i][0][q] + acc[i][1][q];
        v += __shfl_xor(v, 1, 64);
        const int co = co0 + 16 * i + 4 * g4 + q;
        if (!mine || co >= p.Cx) continue;
        const long o = ((long)n * p.Cx + co) * HW + sy * p.W + sx;
        if (pro) v *= silu_grad_f(fmaf(p.x[o], p.gscale[(long)n * p.Cx + co], p.gshift[(long)n * p.Cx + co]));
        p.du[o] = v;
      }
  } else {
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
          if (co >= p.Cx) continue;
          const long o = ((long)n * p.Cx + co) * HW + oy * p.W + ox;
          float v = acc[i][j][q];
          if (pro) v *= silu_grad_f(fmaf(p.x[o], p.gscale[(long)n * p.Cx + co], p.gshift[(long)n * p.Cx + co]));
          p.du[o] = v;
        }
    }
  }
}

// ------------------------------------------------------------------------------------------------ weight gradient
constexpr int kWgTiles = 8;   // pixel tiles a workgroup adds up before it writes its slab

template <int KIND>
struct WGeo {
  static constexpr int TH_ = KIND == 1 ? 4 : 8;                  // tile rows (kind 1: its 9-row patch keeps LDS below the limit)
  static constexpr int PH = KIND == 1 ? 2 * TH_ + 1 : TH_ + 2;   // patch rows
  static constexpr int ROWE = KIND == 1 ? 48 : 24;               // bf16 elements of a patch row: 18 used (kind 1: 2 halves of 17)
  static constexpr int NOCT = ROWE / 8;
  static constexpr int CS = ((PH * ROWE / 8) | 1) * 16;          // bytes of a channel's patch; an odd count of 16-byte pieces
  static constexpr int KT = TH_ * TW;                            // pixels of a tile
  static constexpr int KSTEPS = KT / 32;
  static constexpr int DYS = KT * 2 + 16;                        // bytes of a co row of the dy tile, odd in 16-byte pieces
  static constexpr int A_PLANE = CK * CS, D_PLANE = BM * DYS;
};

struct W3P {
  const float* dy;   // (N, Cout, Ho, Wo)
  const float* x;    // (N, Cin, H, W)
  const float* gscale;
  const float* gshift;
  float* slab;       // [N * G][9][Cout][Cin]
  int N, Cin, Cout, H, W, Ho, Wo, nchunks, tyn, txn, G;
};

// the 8 bf16 of columns c0 + SHIFT .. c0 + SHIFT + 7 out of the two aligned pieces lo (c0 .. c0 + 7) and hi (c0 + 8 ..)
template <int SHIFT>
__device__ __forceinline__ bf16x8 funnel(u32x4 lo, u32x4 hi) {
  u32x4 r;
  if (SHIFT == 0) r = lo;
  else if (SHIFT == 1)
    r = u32x4{(lo[0] >> 16) | (lo[1] << 16), (lo[1] >> 16) | (lo[2] << 16), (lo[2] >> 16) | (lo[3] << 16), (lo[3] >> 16) | (hi[0] << 16)};
  else r = u32x4{lo[1], lo[2], lo[3], hi[0]};
  return __builtin_bit_cast(bf16x8, r);
}

template <int NP>
__device__ __forceinline__ f32x4 mfma_planes(const bf16x8 (&a)[NP], const bf16x8 (&b)[NP], f32x4 c) {
  if constexpr (NP == 3) {   // smallest terms first
    c = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a[2], b[0], c, 0, 0, 0);
    c = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a[0], b[2], c, 0, 0, 0);
    c = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a[1], b[1], c, 0, 0, 0);
    c = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a[1], b[0], c, 0, 0, 0);
    c = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a[0], b[1], c, 0, 0, 0);
  }
  return __builtin_amdgcn_mfma_f32_16x16x32_bf16(a[0], b[0], c, 0, 0, 0);
}

// 8 values -> their bf16 planes, 16 bytes per plane at dst + pl * plane
template <int NP>
__device__ __forceinline__ void store_planes(unsigned char* dst, int plane, const float (&v)[8]) {
  if (NP == 1) {
    *reinterpret_cast<u32x4*>(dst) = u32x4{pack_bf16(v[0], v[1]), pack_bf16(v[2], v[3]), pack_bf16(v[4], v[5]), pack_bf16(v[6], v[7])};
  } else {
    unsigned short h[8], m[8], l[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) split3(v[j], h[j], m[j], l[j]);
    *reinterpret_cast<u32x4*>(dst) = u32x4{WFAE_PK(h, 0), WFAE_PK(h, 2), WFAE_PK(h, 4), WFAE_PK(h, 6)};
    *reinterpret_cast<u32x4*>(dst + plane) = u32x4{WFAE_PK(m, 0), WFAE_PK(m, 2), WFAE_PK(m, 4), WFAE_PK(m, 6)};
    *reinterpret_cast<u32x4*>(dst + 2 * plane) = u32x4{WFAE_PK(l, 0), WFAE_PK(l, 2), WFAE_PK(l, 4), WFAE_PK(l, 6)};
  }
}

template <int KIND, int NP>
__global__ __launch_bounds__(kThreads) void aekl_wgrad_kernel(W3P p) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  using G = WGeo<KIND>;
  constexpr int TH_ = G::TH_, PH = G::PH, ROWE = G::ROWE, NOCT = G::NOCT, CS = G::CS, DYS = G::DYS;
  constexpr int A_PLANE = G::A_PLANE, D_PLANE = G::D_PLANE;
  unsigned char* const sa = smem;                    // [plane][32 ci][PH][ROWE] bf16
  unsigned char* const sd = smem + NP * A_PLANE;     // [plane][64 co][KT] bf16
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6, r15 = lane & 15, g4 = lane >> 4;
  const int co0 = (blockIdx.x / p.nchunks) * BM, ci0 = (blockIdx.x % p.nchunks) * CK;
  const int n = blockIdx.z;
  const int HW = p.H * p.W, HWo = p.Ho * p.Wo;
  const float* __restrict__ xn = p.x + (long)n * p.Cin * HW;
  const float* __restrict__ dyn = p.dy + (long)n * p.Cout * HWo;
  const bool pro = p.gscale != nullptr;
  const float* __restrict__ gs = pro ? p.gscale + (long)n * p.Cin : nullptr;
  const float* __restrict__ gh = pro ? p.gshift + (long)n * p.Cin : nullptr;

  f32x4 acc[2][9];
#pragma unroll
  for (int j = 0; j < 2; ++j)
#pragma unroll
    for (int k = 0; k < 9; ++k)
#pragma unroll
      for (int q = 0; q < 4; ++q) acc[j][k][q] = 0.f;

  const int ntiles = p.tyn * p.txn;
  const int tile_end = min(ntiles, ((int)blockIdx.y + 1) * kWgTiles);
  for (int tile = blockIdx.y * kWgTiles; tile < tile_end; ++tile) {
    const int oy0 = (tile / p.txn) * TH_, ox0 = (tile % p.txn) * TW;
    __syncthreads();   // the fragment reads of the previous tile are done
    // ---- the dy tile: item = (co, tile row, half row of 8 pixels)
    for (int it = t; it < BM * TH_ * 2; it += kThreads) {
      const int o = it & 1, ty = (it >> 1) % TH_, co = it / (2 * TH_);
      const int oy = oy0 + ty, ox = ox0 + 8 * o;
      const bool rok = co0 + co < p.Cout && oy < p.Ho;
      const float* __restrict__ src = dyn + (long)(co0 + co) * HWo + (long)oy * p.Wo + ox;
      float v[8];
#pragma unroll
      for (int e = 0; e < 8; ++e) v[e] = (rok && ox + e < p.Wo) ? src[e] : 0.f;
      store_planes<NP>(sd + co * DYS + (ty * TW + 8 * o) * 2, D_PLANE, v);
    }
    // ---- the patch of a: item = (ci, patch row, piece of 8 columns); prologue on the load, zeros after it
    for (int it = t; it < CK * PH * NOCT; it += kThreads) {
      const int oc = it % NOCT, py = (it / NOCT) % PH, ci = it / (NOCT * PH);
      const bool cok = ci0 + ci < p.Cin;
      const float sc = (pro && cok) ? gs[ci0 + ci] : 1.f, sh = (pro && cok) ? gh[ci0 + ci] : 0.f;
      const float* __restrict__ src = xn + (long)(ci0 + ci) * HW;
      float v[8];
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        int sy, sx;
        bool ok;
        if (KIND == 1) {
          const int half = oc / 3, px = 2 * (8 * (oc % 3) + e) + half;
          sy = 2 * oy0 + py; sx = 2 * ox0 + px;
          ok = px < 2 * TW + 1 && sy < p.H && sx < p.W;
        } else {
          const int col = 8 * oc + e;
          const int uy = oy0 - 1 + py, ux = ox0 - 1 + col;
          const int Hg = KIND == 2 ? 2 * p.H : p.H, Wg = KIND == 2 ? 2 * p.W : p.W;
          ok = col < TW + 2 && uy >= 0 && uy < Hg && ux >= 0 && ux < Wg;
          sy = KIND == 2 ? uy >> 1 : uy; sx = KIND == 2 ? ux >> 1 : ux;
        }
        float val = 0.f;
        if (ok && cok) {
          val = src[(long)sy * p.W + sx];
          if (pro) val = silu_f(fmaf(val, sc, sh));
        }
        v[e] = val;
      }
      store_planes<NP>(sa + ci * CS + (py * ROWE + 8 * oc) * 2, A_PLANE, v);
    }
    __syncthreads();

    f32x4 part[2][9];
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
      for (int k = 0; k < 9; ++k)
#pragma unroll
        for (int q = 0; q < 4; ++q) part[j][k][q] = 0.f;
#pragma unroll
    for (int s = 0; s < G::KSTEPS; ++s) {
      // lane group g4 holds pixels 8 (g4 & 1) .. + 7 of tile row 2 s + (g4 >> 1)
      const int ty = 2 * s + (g4 >> 1), oc = g4 & 1;
      bf16x8 a[NP];
#pragma unroll
      for (int pl = 0; pl < NP; ++pl)
        a[pl] = *reinterpret_cast<const bf16x8*>(sd + pl * D_PLANE + (16 * wave + r15) * DYS + (s * 32 + g4 * 8) * 2);
#pragma unroll
      for (int ky = 0; ky < 3; ++ky)
#pragma unroll
        for (int j = 0; j < 2; ++j) {
          const int row = KIND == 1 ? 2 * ty + ky : ty + ky;
          const unsigned char* base = sa + (16 * j + r15) * CS + (row * ROWE + 8 * oc) * 2;
          u32x4 lo[NP], hi[NP];
          bf16x8 b[NP];
#pragma unroll
          for (int pl = 0; pl < NP; ++pl) {
            lo[pl] = *reinterpret_cast<const u32x4*>(base + pl * A_PLANE);
            hi[pl] = *reinterpret_cast<const u32x4*>(base + pl * A_PLANE + 16);
          }
          if (KIND == 1) {
#pragma unroll
            for (int pl = 0; pl < NP; ++pl) b[pl] = funnel<0>(lo[pl], hi[pl]);
            part[j][3 * ky + 0] = mfma_planes<NP>(a, b, part[j][3 * ky + 0]);
#pragma unroll
            for (int pl = 0; pl < NP; ++pl) b[pl] = funnel<1>(lo[pl], hi[pl]);
            part[j][3 * ky + 2] = mfma_planes<NP>(a, b, part[j][3 * ky + 2]);
#pragma unroll
            for (int pl = 0; pl < NP; ++pl)
              b[pl] = *reinterpret_cast<const bf16x8*>(base + pl * A_PLANE + (ROWE / 2) * 2);   // the odd columns
            part[j][3 * ky + 1] = mfma_planes<NP>(a, b, part[j][3 * ky + 1]);
          } else {
#pragma unroll
            for (int pl = 0; pl < NP; ++pl) b[pl] = funnel<0>(lo[pl], hi[pl]);
            part[j][3 * ky + 0] = mfma_planes<NP>(a, b, part[j][3 * ky + 0]);
#pragma unroll
            for (int pl = 0; pl < NP; ++pl) b[pl] = funnel<1>(lo[pl], hi[pl]);
            part[j][3 * ky + 1] = mfma_planes<NP>(a, b, part[j][3 * ky + 1]);
#pragma unroll
            for (int pl = 0; pl < NP; ++pl) b[pl] = funnel<2>(lo[pl], hi[pl]);
            part[j][3 * ky + 2] = mfma_planes<NP>(a, b, part[j][3 * ky + 2]);
          }
        }
    }
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
      for (int k = 0; k < 9; ++k) acc[j][k] += part[j][k];
  }

  // ---- the slab: register q of lane (r15, g4) of tile (j, tap) is (co = 16 wave + 4 g4 + q, ci = 16 j + r15)
  float* __restrict__ out = p.slab + ((long)n * p.G + blockIdx.y) * 9 * p.Cout * p.Cin;
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    const int ci = ci0 + 16 * j + r15;
    if (ci >= p.Cin) continue;
#pragma unroll
    for (int k = 0; k < 9; ++k)
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const int co = co0 + 16 * wave + 4 * g4 + q;
        if (co < p.Cout) out[((long)k * p.Cout + co) * p.Cin + ci] = acc[j][k][q];
      }
  }
}

// dW[co][ci][tap] = the slabs [s][tap][co][ci] added in ascending order
__global__ __launch_bounds__(256) void aekl_wgrad_final_kernel(const float* __restrict__ slab, float* __restrict__ dw, long CC,
                                                               int slabs) {
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= 9 * CC) return;
  const long tap = i / CC, r = i - tap * CC;
  double s = 0.0;
  for (int b = 0; b < slabs; ++b) s += (double)slab[(long)b * 9 * CC + i];
  dw[r * 9 + tap] = (float)s;
}

// dbias[c] = sum over samples and pixels of dy; one workgroup per channel, fp64 partials, fixed order
__global__ __launch_bounds__(256) void aekl_dbias_kernel(const float* __restrict__ dy, float* __restrict__ dbias, int N, int C,
                                                         long HW) {
  __shared__ double red[16];
  const int c = blockIdx.x;
  double s = 0.0;
  for (int n = 0; n < N; ++n) {
    const float* __restrict__ src = dy + ((long)n * C + c) * HW;
    for (long i = threadIdx.x; i < HW; i += 256) s += (double)src[i];
  }
  s = block_sum(s, red);
  if (threadIdx.x == 0) dbias[c] = (float)s;
}

// ------------------------------------------------------------------------------------------------ GroupNorm backward
// part[(n C + c) 2 + {0, 1}] = sum over the pixels of du, of du xhat
__global__ __launch_bounds__(256) void aekl_gn_bwd_part_kernel(const float* __restrict__ du, const float* __restrict__ x,
                                                               const float* __restrict__ mean, const float* __restrict__ rstd,
                                                               double* __restrict__ part, int C, int G, long HW) {
  __shared__ double red[16];
  const long nc = blockIdx.x;
  const int n = (int)(nc / C), c = (int)(nc % C);
  const float mu = mean[n * G + c / (C / G)], rs = rstd[n * G + c / (C / G)];
  const float* __restrict__ d = du + nc * HW;
  const float* __restrict__ xs = x + nc * HW;
  double a = 0.0, b = 0.0;
  for (long i = threadIdx.x; i < HW; i += 256) {
    const float g = d[i];
    a += (double)g;
    b += (double)(g * ((xs[i] - mu) * rs));
  }
  a = block_sum(a, red);
  b = block_sum(b, red);
  if (threadIdx.x == 0) {
    part[2 * nc] = a;
    part[2 * nc + 1] = b;
  }
}

// blocks [0, N G): gsum[ng] = (s1, s2) over the group's channels in ascending order; the blocks behind them: dbeta, dgamma
// of 256 channels each over the samples in ascending order
__global__ __launch_bounds__(256) void aekl_gn_bwd_final_kernel(const double* __restrict__ part, const float* __restrict__ gamma,
                                                                double* __restrict__ gsum, float* __restrict__ dgamma,
                                                                float* __restrict__ dbeta, int N, int C, int G) {
  const int NG = N * G, Cg = C / G;
  if ((int)blockIdx.x < NG) {
    if (threadIdx.x) return;
    const int n = blockIdx.x / G, g = blockIdx.x % G;
    double s1 = 0.0, s2 = 0.0;
    for (int c = g * Cg; c < (g + 1) * Cg; ++c) {
      const double gm = (double)gamma[c];
      s1 += gm * part[2 * ((long)n * C + c)];
      s2 += gm * part[2 * ((long)n * C + c) + 1];
    }
    gsum[2 * blockIdx.x] = s1;
    gsum[2 * blockIdx.x + 1] = s2;
    return;
  }
  const int c = ((int)blockIdx.x - NG) * 256 + threadIdx.x;
  if (c >= C) return;
  double a = 0.0, b = 0.0;
  for (int n = 0; n < N; ++n) {
    a += part[2 * ((long)n * C + c)];
    b += part[2 * ((long)n * C + c) + 1];
  }
  dbeta[c] = (float)a;
  dgamma[c] = (float)b;
}

// dx = rstd (du gamma_c - (s1 + xhat s2) / m) + skip
__global__ __launch_bounds__(256) void aekl_gn_bwd_apply_kernel(const float* __restrict__ du, const float* __restrict__ x,
                                                                const float* __restrict__ gamma, const float* __restrict__ mean,
                                                                const float* __restrict__ rstd, const double* __restrict__ gsum,
                                                                const float* __restrict__ skip, float* __restrict__ dx, int C,
                                                                int G, long HW) {
  const long nc = blockIdx.y;
  const int n = (int)(nc / C), c = (int)(nc % C), ng = n * G + c / (C / G);
  const float mu = mean[ng], rs = rstd[ng], gm = gamma[c];
  const double m = (double)(C / G) * (double)HW;
  const float k1 = (float)(gsum[2 * ng] / m), k2 = (float)(gsum[2 * ng + 1] / m);
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < HW; i += (long)gridDim.x * 256) {
    const long o = nc * HW + i;
    const float xh = (x[o] - mu) * rs;
    float v = rs * (fmaf(du[o], gm, -k1) - xh * k2);
    if (skip) v += skip[o];
    dx[o] = v;
  }
}

// ds[row] = p (dp - sum_j p_j dp_j) scale; one workgroup per row
__global__ __launch_bounds__(256) void aekl_softmax_bwd_kernel(const float* __restrict__ p, const float* __restrict__ dp,
                                                               float* __restrict__ ds, int cols, float scale) {
  __shared__ double red[16];
  __shared__ double bc;
  const float* __restrict__ pr = p + (long)blockIdx.x * cols;
  const float* __restrict__ dr = dp + (long)blockIdx.x * cols;
  float* __restrict__ sr = ds + (long)blockIdx.x * cols;
  double s = 0.0;
  for (int i = threadIdx.x; i < cols; i += 256) s += (double)(pr[i] * dr[i]);
  const float dot = (float)block_sum_all(s, red, &bc);
  for (int i = threadIdx.x; i < cols; i += 256) sr[i] = pr[i] * (dr[i] - dot) * scale;
}

// dmoments (N, 2C, HW) from dz (may be null), the noise (may be null: z was the mean) and the per-sample KL gradient gkl
// (may be null)
__global__ __launch_bounds__(256) void aekl_posterior_bwd_kernel(const float* __restrict__ dz, const float* __restrict__ noise,
                                                                 const float* __restrict__ mom, const float* __restrict__ gkl,
                                                                 float* __restrict__ dmom, long CHW, long total) {
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= total) return;
  const long n = i / CHW, r = i - n * CHW;
  const float mu = mom[n * 2 * CHW + r], raw = mom[n * 2 * CHW + CHW + r];
  const float lv = fminf(fmaxf(raw, -30.0f), 20.0f);
  const float sd = expf(0.5f * lv);
  const float g = dz ? dz[i] : 0.f, k = gkl ? gkl[n] : 0.f;
  float dl = 0.f;
  if (noise) dl = 0.5f * g * noise[i] * sd;
  dl = fmaf(0.5f * k, fmaf(sd, sd, -1.0f), dl);
  if (!(raw >= -30.0f && raw <= 20.0f)) dl = 0.f;
  dmom[n * 2 * CHW + r] = fmaf(k, mu, g);
  dmom[n * 2 * CHW + CHW + r] = dl;
}

#undef WFAE_PK

inline int pad_to(int v, int m) { return (v + m - 1) / m * m; }

template <int KIND, int MODE>
int launch_dgrad(const D3P& p, int Hg, int Wg, hipStream_t st) {
  constexpr size_t lds = (size_t)DPP * Rec<MODE>::B * (MODE == MODE_SPLIT3 ? 3 : 1);
  static_assert(lds <= 64 * 1024, "patch does not fit LDS");
  const dim3 grid(cdiv(Wg, TW), cdiv(Hg, TH), p.N * p.ncb);
  hipLaunchKernelGGL((aekl_dgrad_kernel<KIND, MODE>), grid, dim3(kThreads), lds, st, p);
  return check_launch("aekl_conv3_bwd_data");
}

template <int KIND>
int launch_dgrad_mode(const D3P& p, int mode, int Hg, int Wg, hipStream_t st) {
  if (mode == MODE_BF16) return launch_dgrad<KIND, MODE_BF16>(p, Hg, Wg, st);
  if (mode == MODE_SPLIT3) return launch_dgrad<KIND, MODE_SPLIT3>(p, Hg, Wg, st);
  return launch_dgrad<KIND, MODE_F32>(p, Hg, Wg, st);
}

template <int KIND, int NP>
int launch_wgrad(const W3P& p, hipStream_t st) {
  using G = WGeo<KIND>;
  constexpr size_t lds = (size_t)NP * (G::A_PLANE + G::D_PLANE);
  static_assert(lds <= kLdsLimit, "tiles do not fit LDS");
  static_assert(G::CS >= G::PH * G::ROWE * 2 && G::CS % 16 == 0 && G::DYS % 16 == 0, "LDS rows");
  (void)hipFuncSetAttribute((const void*)aekl_wgrad_kernel<KIND, NP>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)kLdsLimit);
  const dim3 grid(p.nchunks * (pad_to(p.Cout, BM) / BM), p.G, p.N);
  hipLaunchKernelGGL((aekl_wgrad_kernel<KIND, NP>), grid, dim3(kThreads), lds, st, p);
  return check_launch("aekl_conv3_bwd_weight");
}

inline void out_plane(int kind, int H, int W, int* Ho, int* Wo) {
  *Ho = kind == 0 ? H : kind == 1 ? (H - 2) / 2 + 1 : 2 * H;
  *Wo = kind == 0 ? W : kind == 1 ? (W - 2) / 2 + 1 : 2 * W;
}
inline int wgrad_groups(int kind, int Ho, int Wo) {
  const int th = kind == 1 ? WGeo<1>::TH_ : WGeo<0>::TH_;
  return cdiv((long)cdiv(Ho, th) * cdiv(Wo, TW), kWgTiles);
}
inline bool conv_shape_ok(int kind, int N, int H, int W) {
  return N > 0 && H > 0 && W > 0 && H <= 8192 && W <= 8192 && (kind != 1 || (H >= 2 && W >= 2));
}

}  // namespace

extern "C" {

int wfae_aekl_conv3_bwd_data(const float* dy, const void* packed_t, const float* x, const float* gn_scale, const float* gn_shift,
                             float* du, int kind, int mode, int N, int Cin, int Cout, int H, int W, wfae_stream_t stream) {
  WFAE_REQUIRE(dy && packed_t && du, WFAE_ERR_NULL_POINTER, "aekl_conv3_bwd_data: null pointer");
  WFAE_REQUIRE((gn_scale == nullptr) == (gn_shift == nullptr) && (gn_scale == nullptr || x), WFAE_ERR_NULL_POINTER,
               "aekl_conv3_bwd_data: the prologue factor needs x, gn_scale and gn_shift");
  WFAE_REQUIRE(kind >= 0 && kind <= 2, WFAE_ERR_BAD_SHAPE, "aekl_conv3_bwd_data: kind %d (0, 1 or 2 as in aekl_conv3_fwd)", kind);
  WFAE_REQUIRE(mode == MODE_BF16 || mode == MODE_SPLIT3 || mode == MODE_F32, WFAE_ERR_BAD_SHAPE,
               "aekl_conv3_bwd_data: mode %d (1 = bf16, 3 = three bf16 planes, 4 = fp32)", mode);
  WFAE_REQUIRE(conv_shape_ok(kind, N, H, W), WFAE_ERR_BAD_SHAPE, "aekl_conv3_bwd_data: bad shape N=%d H=%d W=%d", N, H, W);
  WFAE_REQUIRE(Cout > 0 && Cin > 0 && Cout <= 4096 && Cin <= 4096, WFAE_ERR_UNSUPPORTED,
               "aekl_conv3_bwd_data: channel counts 1..4096 are served (got Cout=%d Cin=%d)", Cout, Cin);
  WFAE_REQUIRE((reinterpret_cast<uintptr_t>(packed_t) & 15) == 0, WFAE_ERR_BAD_SHAPE, "aekl_conv3_bwd_data: packed_t must be 16-byte aligned");
  D3P p = {};
  p.dy = dy; p.w = packed_t; p.x = x; p.gscale = gn_scale; p.gshift = gn_shift; p.du = du;
  p.N = N; p.Cd = Cout; p.Cx = Cin; p.H = H; p.W = W;
  out_plane(kind, H, W, &p.Hd, &p.Wd);
  p.CxP = pad_to(Cin, BM);
  p.ncb = p.CxP / BM;
  p.nchunks = pad_to(Cout, CK) / CK;
  WFAE_REQUIRE((long)Cin * H * W < (1l << 31) && (long)Cout * p.Hd * p.Wd < (1l << 31), WFAE_ERR_BAD_SHAPE,
               "aekl_conv3_bwd_data: one sample must stay below 2^31 elements");
  const int Hg = kind == 2 ? 2 * H : H, Wg = kind == 2 ? 2 * W : W;   // the grid the tiles cover
  WFAE_REQUIRE((long)N * p.ncb <= 65535 && cdiv(Hg, TH) <= 65535, WFAE_ERR_BAD_SHAPE, "aekl_conv3_bwd_data: grid too large");
  hipStream_t st = (hipStream_t)stream;
  if (kind == 0) return launch_dgrad_mode<0>(p, mode, Hg, Wg, st);
  if (kind == 1) return launch_dgrad_mode<1>(p, mode, Hg, Wg, st);
  return launch_dgrad_mode<2>(p, mode, Hg, Wg, st);
}

size_t wfae_aekl_conv3_wgrad_ws_bytes(int kind, int N, int Cin, int Cout, int H, int W) {
  if (kind < 0 || kind > 2 || !conv_shape_ok(kind, N, H, W) || Cin <= 0 || Cout <= 0 || Cin > 4096 || Cout > 4096) return 0;
  int Ho, Wo;
  out_plane(kind, H, W, &Ho, &Wo);
  return (size_t)N * wgrad_groups(kind, Ho, Wo) * 9 * Cout * Cin * sizeof(float);
}

int wfae_aekl_conv3_bwd_weight(const float* dy, const float* x, const float* gn_scale, const float* gn_shift, float* dw,
                               float* dbias, int kind, int mode, int N, int Cin, int Cout, int H, int W, void* ws,
                               size_t ws_bytes, wfae_stream_t stream) {
  WFAE_REQUIRE(dy && x && dw, WFAE_ERR_NULL_POINTER, "aekl_conv3_bwd_weight: null pointer");
  WFAE_REQUIRE((gn_scale == nullptr) == (gn_shift == nullptr), WFAE_ERR_NULL_POINTER,
               "aekl_conv3_bwd_weight: the prologue needs both gn_scale and gn_shift");
  WFAE_REQUIRE(kind >= 0 && kind <= 2, WFAE_ERR_BAD_SHAPE, "aekl_conv3_bwd_weight: kind %d (0, 1 or 2 as in aekl_conv3_fwd)", kind);
  WFAE_REQUIRE(mode == MODE_BF16 || mode == MODE_SPLIT3 || mode == MODE_F32, WFAE_ERR_BAD_SHAPE,
               "aekl_conv3_bwd_weight: mode %d (1 = bf16, 3 = three bf16 planes)", mode);
  WFAE_REQUIRE(mode != MODE_F32, WFAE_ERR_UNSUPPORTED, "aekl_conv3_bwd_weight: mode 4 (fp32 operands) is not built; use 3");
  WFAE_REQUIRE(conv_shape_ok(kind, N, H, W) && N <= 65535, WFAE_ERR_BAD_SHAPE, "aekl_conv3_bwd_weight: bad shape N=%d H=%d W=%d", N, H, W);
  WFAE_REQUIRE(Cout > 0 && Cin > 0 && Cout <= 4096 && Cin <= 4096, WFAE_ERR_UNSUPPORTED,
               "aekl_conv3_bwd_weight: channel counts 1..4096 are served (got Cout=%d Cin=%d)", Cout, Cin);
  W3P p = {};
  p.dy = dy; p.x = x; p.gscale = gn_scale; p.gshift = gn_shift; p.slab = (float*)ws;
  p.N = N; p.Cin = Cin; p.Cout = Cout; p.H = H; p.W = W;
  out_plane(kind, H, W, &p.Ho, &p.Wo);
  WFAE_REQUIRE((long)Cin * H * W < (1l << 31) && (long)Cout * p.Ho * p.Wo < (1l << 31), WFAE_ERR_BAD_SHAPE,
               "aekl_conv3_bwd_weight: one sample must stay below 2^31 elements");
  p.nchunks = pad_to(Cin, CK) / CK;
  p.tyn = cdiv(p.Ho, kind == 1 ? WGeo<1>::TH_ : WGeo<0>::TH_);
  p.txn = cdiv(p.Wo, TW);
  p.G = wgrad_groups(kind, p.Ho, p.Wo);
  WFAE_REQUIRE(p.G <= 65535, WFAE_ERR_BAD_SHAPE, "aekl_conv3_bwd_weight: grid too large");
  const size_t need = wfae_aekl_conv3_wgrad_ws_bytes(kind, N, Cin, Cout, H, W);
  WFAE_REQUIRE(ws && ws_bytes >= need, WFAE_ERR_WORKSPACE, "aekl_conv3_bwd_weight: workspace too small (%zu < %zu)", ws_bytes, need);
  WFAE_REQUIRE((reinterpret_cast<uintptr_t>(ws) & 15) == 0, WFAE_ERR_WORKSPACE, "aekl_conv3_bwd_weight: workspace must be 16-byte aligned");
  hipStream_t st = (hipStream_t)stream;
  int rc;
  if (mode == MODE_SPLIT3)
    rc = kind == 0 ? launch_wgrad<0, 3>(p, st) : kind == 1 ? launch_wgrad<1, 3>(p, st) : launch_wgrad<2, 3>(p, st);
  else
    rc = kind == 0 ? launch_wgrad<0, 1>(p, st) : kind == 1 ? launch_wgrad<1, 1>(p, st) : launch_wgrad<2, 1>(p, st);
  if (rc) return rc;
  const long CC = (long)Cout * Cin;
  hipLaunchKernelGGL(aekl_wgrad_final_kernel, dim3((unsigned)((9 * CC + 255) / 256)), dim3(256), 0, st, (const float*)ws, dw, CC,
                     N * p.G);
  rc = check_launch("aekl_conv3_bwd_weight_final");
  if (rc || !dbias) return rc;
  hipLaunchKernelGGL(aekl_dbias_kernel, dim3(Cout), dim3(256), 0, st, dy, dbias, N, Cout, (long)p.Ho * p.Wo);
  return check_launch("aekl_conv3_bwd_bias");
}

size_t wfae_aekl_gn_bwd_ws_bytes(int N, int C, int groups) {
  if (N <= 0 || C <= 0 || groups <= 0 || C % groups) return 0;
  return ((size_t)N * C + (size_t)N * groups) * 2 * sizeof(double);
}

int wfae_aekl_gn_bwd(const float* du, const float* x, const float* gamma, const float* mean, const float* rstd, const float* skip,
                     float* dx, float* dgamma, float* dbeta, int N, int C, int HW, int groups, void* ws, size_t ws_bytes,
                     wfae_stream_t stream) {
  WFAE_REQUIRE(du && x && gamma && mean && rstd && dx && dgamma && dbeta, WFAE_ERR_NULL_POINTER, "aekl_gn_bwd: null pointer");
  WFAE_REQUIRE(N > 0 && C > 0 && HW > 0 && groups > 0 && C % groups == 0, WFAE_ERR_BAD_SHAPE,
               "aekl_gn_bwd: bad shape N=%d C=%d HW=%d groups=%d", N, C, HW, groups);
  WFAE_REQUIRE((long)N * C <= 65535, WFAE_ERR_BAD_SHAPE, "aekl_gn_bwd: N * C = %ld > 65535", (long)N * C);
  const size_t need = wfae_aekl_gn_bwd_ws_bytes(N, C, groups);
  WFAE_REQUIRE(ws && ws_bytes >= need, WFAE_ERR_WORKSPACE, "aekl_gn_bwd: workspace too small (%zu < %zu)", ws_bytes, need);
  WFAE_REQUIRE((reinterpret_cast<uintptr_t>(ws) & 7) == 0, WFAE_ERR_WORKSPACE, "aekl_gn_bwd: workspace must be 8-byte aligned");
  hipStream_t st = (hipStream_t)stream;
  double* part = (double*)ws;
  double* gsum = part + (size_t)N * C * 2;
  hipLaunchKernelGGL(aekl_gn_bwd_part_kernel, dim3(N * C), dim3(256), 0, st, du, x, mean, rstd, part, C, groups, (long)HW);
  int rc = check_launch("aekl_gn_bwd_part");
  if (rc) return rc;
  hipLaunchKernelGGL(aekl_gn_bwd_final_kernel, dim3(N * groups + cdiv(C, 256)), dim3(256), 0, st, (const double*)part, gamma, gsum,
                     dgamma, dbeta, N, C, groups);
  rc = check_launch("aekl_gn_bwd_final");
  if (rc) return rc;
  const int bx = HW >= 4096 ? 4 : 1;
  hipLaunchKernelGGL(aekl_gn_bwd_apply_kernel, dim3(bx, N * C), dim3(256), 0, st, du, x, gamma, mean, rstd, (const double*)gsum, skip,
                     dx, C, groups, (long)HW);
  return check_launch("aekl_gn_bwd_apply");
}

int wfae_aekl_softmax_bwd(const float* p, const float* dp, float* ds, int64_t rows, int cols, float scale, wfae_stream_t stream) {
  WFAE_REQUIRE(p && dp && ds, WFAE_ERR_NULL_POINTER, "aekl_softmax_bwd: null pointer");
  WFAE_REQUIRE(rows > 0 && rows < (1ll << 31) && cols > 0, WFAE_ERR_BAD_SHAPE, "aekl_softmax_bwd: bad shape");
  hipLaunchKernelGGL(aekl_softmax_bwd_kernel, dim3((unsigned)rows), dim3(256), 0, (hipStream_t)stream, p, dp, ds, cols, scale);
  return check_launch("aekl_softmax_bwd");
}

int wfae_aekl_posterior_bwd(const float* dz, const float* noise, const float* moments, const float* gkl, float* dmoments, int N,
                            int C, int HW, wfae_stream_t stream) {
  WFAE_REQUIRE(moments && dmoments, WFAE_ERR_NULL_POINTER, "aekl_posterior_bwd: null pointer");
  WFAE_REQUIRE(dz || !noise, WFAE_ERR_NULL_POINTER, "aekl_posterior_bwd: noise without dz");
  WFAE_REQUIRE(N > 0 && C > 0 && HW > 0, WFAE_ERR_BAD_SHAPE, "aekl_posterior_bwd: bad shape N=%d C=%d HW=%d", N, C, HW);
  const long CHW = (long)C * HW, total = CHW * N;
  WFAE_REQUIRE(total < (1l << 39), WFAE_ERR_BAD_SHAPE, "aekl_posterior_bwd: too large");
  hipLaunchKernelGGL(aekl_posterior_bwd_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream, dz, noise,
                     moments, gkl, dmoments, CHW, total);
  return check_launch("aekl_posterior_bwd");
}

}  // extern "C"
