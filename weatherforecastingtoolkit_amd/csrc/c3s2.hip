// c3s2.hip — the 3x3, stride 2, padding 1 convolution family of the conv + GAN latent model (reference
// experiments/v1_experiments/pretrained_ae_conv_disc/train.py:140-206 `Encoder`, `Decoder`): Conv2d + bias + SiLU and
// ConvTranspose2d(output_padding 0 / 1) + bias + SiLU, forward, data gradient and weight gradient, plain fp32 on the VALU.
//
// One weight layout serves both module types: w[Clo][Chi][3][3] is Conv2d(Chi -> Clo).weight and
// ConvTranspose2d(Clo -> Chi).weight.  "hi" is the larger plane, "lo" the smaller: Hlo = (Hhi - 1) / 2 + 1.  Three forms:
//   gather   lo[n][cl][oy][ox]  = sum_{ch,ky,kx} w[cl][ch][ky][kx] hi[n][ch][2 oy - 1 + ky][2 ox - 1 + kx]
//   scatter  hi[n][ch][iy][ix]  = sum_{cl,ky,kx : iy = 2 oy - 1 + ky, ix = 2 ox - 1 + kx} w[cl][ch][ky][kx] lo[n][cl][oy][ox]
//   wgrad    dw[cl][ch][ky][kx] = sum_{n,oy,ox} lo[n][cl][oy][ox] hi[n][ch][2 oy - 1 + ky][2 ox - 1 + kx]
// Conv2d: forward = gather, data gradient = scatter; ConvTranspose2d: forward = scatter, data gradient = gather.
//
// The regime (batch 8: 8 .. 2048 rows against 0.3 .. 37.7 MB of weights) is weight streaming, so every kernel is
// weight-stationary: a lane owns four consecutive floats of a weight row (one 16-byte access, a wavefront one KiB of
// contiguous weights), reads them once and applies them to a tile of 8 rows of the small activation held in LDS.
//   gather:  the contiguous index of a weight row is the reduction index k = (ch, tap).  The 8 x 256 im2col tile of the
//            activation is staged in LDS as A[row][k]; a lane's 16-byte LDS read is the four k of its four weights (no bank
//            conflicts); a wavefront keeps 8 weight rows x 8 activation rows of partial sums per lane and folds the 64 lanes
//            once, after its last K chunk.
//   scatter: the contiguous index m = (ch, tap) is an OUTPUT index: P[m][r] = sum_cl w[cl][m] lo[cl][r] is a product with no
//            cross-lane sum (lo values are LDS broadcasts), and hi is the col2im of P, taken by the finishing kernel — each hi
//            pixel reads the 1, 2 or 4 taps of its row / column parity.
//   wgrad:   output-stationary on the same contiguous index m: dw[cl][m] += lo[cl][r] A[r][m] over the rows r.
// Few rows against many weights leaves few output tiles, so the reduction (K chunks, cl ranges, row ranges) is split over
// workgroups as well; the partial sums go to the workspace and a second kernel adds them in ascending order (and applies
// bias + SiLU, or the col2im).  No atomics: two launches on the same inputs give the same bits.
//
// Dead taps: tap (ky, kx) is live only if some lo position reads a real hi pixel through it.  At 2x2 -> 1x1 five of the nine
// taps are dead.  Their weights never enter the arithmetic (they are replaced by 0 before the first multiply, so a NaN
// there stays there), and their gradients are written as exact zeros, or left alone when accumulating.
//
// dt = da SiLU'(t) of the backward passes is formed where da is read (the LDS staging), never by a launch of its own; the
// bias gradient comes from extra workgroups of the weight-gradient launch.
#include "common.h"

using namespace wfae;

namespace {

constexpr int kThreads = 256;
constexpr int kRT = 8;          // activation rows per tile
constexpr int kKC = 256;        // contiguous weight floats per wavefront step: 64 lanes x 4
constexpr int kClw = 8;         // weight rows per wavefront (gather, wgrad)
constexpr int kClt = 32;        // weight rows per workgroup (gather, wgrad)
constexpr int kSCl = 512;       // cl range of one scatter workgroup (its lo tile is held in LDS)
constexpr int kTargetBlocks = 512;

struct Geo {
  int N, Chi, Clo, Hhi, Whi, Hlo, Wlo;
  int live;                     // bit ky * 3 + kx
};

__host__ __device__ inline int live_axis(int k, int hi, int lo) {   // some o in [0, lo): 0 <= 2 o - 1 + k < hi
  for (int o = 0; o < lo && o < 2; ++o) {                           // o = 0 serves k = 1, 2; o = 1 serves k = 0
    const int s = 2 * o - 1 + k;
    if (s >= 0 && s < hi) return 1;
  }
  return 0;
}
__host__ __device__ inline int live_mask(int Hhi, int Whi, int Hlo, int Wlo) {
  int m = 0;
  for (int ky = 0; ky < 3; ++ky)
    for (int kx = 0; kx < 3; ++kx)
      if (live_axis(ky, Hhi, Hlo) && live_axis(kx, Whi, Wlo)) m |= 1 << (ky * 3 + kx);
  return m;
}

__device__ __forceinline__ float silu_f(float t) { return t * sigmoid_f(t); }
__device__ __forceinline__ float silu_grad_f(float t) {
  const float s = sigmoid_f(t);
  return s * fmaf(t, 1.0f - s, 1.0f);
}
// the value of a backward operand: da SiLU'(t) where t is given, else the tensor itself
__device__ __forceinline__ float src_val(const float* __restrict__ v, const float* __restrict__ t, long i) {
  const float a = v[i];
  return t ? a * silu_grad_f(t[i]) : a;
}

// four consecutive weights w[base .. base + 3] of a row that ends at `end`; vec: base is 16-byte aligned
__device__ __forceinline__ void load_w4(const float* __restrict__ w, long base, long end, bool vec, float (&o)[4]) {
  if (vec && base + 3 < end) {
    const float4 v = *reinterpret_cast<const float4*>(w + base);
    o[0] = v.x; o[1] = v.y; o[2] = v.z; o[3] = v.w;
  } else {
#pragma unroll
    for (int j = 0; j < 4; ++j) o[j] = base + j < end ? w[base + j] : 0.f;
  }
}

// row r of the lo side -> {n, 2 oy - 1, 2 ox - 1, valid}
__device__ __forceinline__ int4 row_info(long r, long R, const Geo& g) {
  if (r >= R) return make_int4(0, 0, 0, 0);
  const int HWlo = g.Hlo * g.Wlo;
  const int n = (int)(r / HWlo), p = (int)(r % HWlo);
  return make_int4(n, 2 * (p / g.Wlo) - 1, 2 * (p % g.Wlo) - 1, 1);
}

// A[row][kk] (kk = threadIdx.x: one (ch, tap) per thread) of 8 rows: the hi pixel row `ri` reads through tap (ky, kx)
__device__ __forceinline__ void stage_im2col(float* A, const int4* ri, const float* __restrict__ hi,
                                             const float* __restrict__ thi, const Geo& g, int ch, int ky, int kx, bool kvalid) {
  const long HWhi = (long)g.Hhi * g.Whi;
#pragma unroll
  for (int r = 0; r < kRT; ++r) {
    const int4 q = ri[r];
    const int iy = q.y + ky, ix = q.z + kx;
    float v = 0.f;
    if (kvalid && q.w && iy >= 0 && iy < g.Hhi && ix >= 0 && ix < g.Whi)
      v = src_val(hi, thi, ((long)q.x * g.Chi + ch) * HWhi + (long)iy * g.Whi + ix);
    A[r * kKC + threadIdx.x] = v;
  }
}

// ---- gather: part[z][cl][r] = sum over the K chunks of split z
__global__ __launch_bounds__(kThreads) void wfae_c3s2_gather_kernel(const float* __restrict__ hi, const float* __restrict__ thi,
                                                                    const float* __restrict__ w, float* __restrict__ part,
                                                                    Geo g, long R, int chunks_per_split, bool vec) {
  __shared__ __attribute__((aligned(16))) float A[kRT * kKC];
  __shared__ int4 ri[kRT];
  const int K = g.Chi * 9, nch = (K + kKC - 1) / kKC;
  const int cl0 = blockIdx.x * kClt;
  const long r0 = (long)blockIdx.y * kRT;
  const int z = blockIdx.z;
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  if (threadIdx.x < kRT) ri[threadIdx.x] = row_info(r0 + threadIdx.x, R, g);
  float acc[kClw][kRT];
#pragma unroll
  for (int i = 0; i < kClw; ++i)
#pragma unroll
    for (int r = 0; r < kRT; ++r) acc[i][r] = 0.f;
  const int c_end = min(nch, (z + 1) * chunks_per_split);
  for (int c = z * chunks_per_split; c < c_end; ++c) {
    const int k0 = c * kKC;
    __syncthreads();   // the row table (first pass), the previous tile's readers (later ones)
    {
      const int k = k0 + threadIdx.x, tap = k % 9;
      stage_im2col(A, ri, hi, thi, g, k / 9, tap / 3, tap % 3, k < K);
    }
    __syncthreads();
    float a[kRT][4];
#pragma unroll
    for (int r = 0; r < kRT; ++r) {
      const float4 v = *reinterpret_cast<const float4*>(A + r * kKC + 4 * lane);
      a[r][0] = v.x; a[r][1] = v.y; a[r][2] = v.z; a[r][3] = v.w;
    }
    bool lv[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) lv[j] = (g.live >> ((k0 + 4 * lane + j) % 9)) & 1;
#pragma unroll
    for (int i = 0; i < kClw; ++i) {
      const int cl = cl0 + wv * kClw + i;
      if (cl < g.Clo) {   // wave-uniform
        float wq[4];
        load_w4(w, (long)cl * K + k0 + 4 * lane, (long)(cl + 1) * K, vec, wq);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const float wj = lv[j] ? wq[j] : 0.f;   // a dead tap's weight never enters the arithmetic
#pragma unroll
          for (int r = 0; r < kRT; ++r) acc[i][r] = fmaf(wj, a[r][j], acc[i][r]);
        }
      }
    }
  }
  // fold the 64 lanes; lane i * 8 + r keeps sum (i, r) and stores it
  float mine = 0.f;
#pragma unroll
  for (int i = 0; i < kClw; ++i)
#pragma unroll
    for (int r = 0; r < kRT; ++r) {
      const float s = wave_sum(acc[i][r]);
      if (lane == i * kRT + r) mine = s;
    }
  const int cl = cl0 + wv * kClw + lane / kRT;
  const long r = r0 + lane % kRT;
  if (cl < g.Clo && r < R) part[((long)z * g.Clo + cl) * R + r] = mine;
}

// out[n][c][p] = act(sum_z part[z][c][r] + bias[c]); t (may be null) takes the pre-activation
__global__ __launch_bounds__(256) void wfae_c3s2_gather_final_kernel(const float* __restrict__ part, const float* __restrict__ bias,
                                                                     float* __restrict__ y, float* __restrict__ t, int C, long R,
                                                                     int HW, int splits, int act) {
  const long total = (long)C * R;
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
    const int c = (int)(i / R);
    const long r = i % R;
    float s = 0.f;
    for (int z = 0; z < splits; ++z) s += part[(long)z * total + i];
    if (bias) s += bias[c];
    const long o = ((r / HW) * C + c) * HW + r % HW;
    if (t) t[o] = s;
    y[o] = act ? silu_f(s) : s;
  }
}

// ---- scatter: P[z][m][r] = sum over the cl range of split z of w[cl][m] lo[cl][r];  m = (ch, tap)
__global__ __launch_bounds__(kThreads) void wfae_c3s2_scatter_kernel(const float* __restrict__ lo, const float* __restrict__ tlo,
                                                                     const float* __restrict__ w, float* __restrict__ P, Geo g,
                                                                     long R, int cl_per_split, bool vec) {
  __shared__ __attribute__((aligned(16))) float L[3 * kKC * kRT];   // the lo tile [cl][8] (<= 512 x 8), then the wave sums
  const int M = g.Chi * 9, HWlo = g.Hlo * g.Wlo;
  const int m0 = blockIdx.x * kKC;
  const long r0 = (long)blockIdx.y * kRT;
  const int z = blockIdx.z;
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int clb = z * cl_per_split, cnt = min(g.Clo, clb + cl_per_split) - clb;
  for (int i = threadIdx.x; i < cnt * kRT; i += kThreads) {
    const int c = i / kRT;
    const long r = r0 + i % kRT;
    L[i] = r < R ? src_val(lo, tlo, ((r / HWlo) * g.Clo + clb + c) * HWlo + r % HWlo) : 0.f;
  }
  __syncthreads();
  const int m = m0 + 4 * lane;
  bool lv[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) lv[j] = (g.live >> ((m + j) % 9)) & 1;
  float acc[4][kRT];
#pragma unroll
  for (int j = 0; j < 4; ++j)
#pragma unroll
    for (int r = 0; r < kRT; ++r) acc[j][r] = 0.f;
  const int per_wave = (cnt + 3) / 4;
  const int c_end = min(cnt, (wv + 1) * per_wave);
#pragma unroll 4
  for (int c = wv * per_wave; c < c_end; ++c) {
    float wq[4];
    load_w4(w, (long)(clb + c) * M + m, (long)(clb + c + 1) * M, vec, wq);
    const float4 a0 = *reinterpret_cast<const float4*>(L + c * kRT);
    const float4 a1 = *reinterpret_cast<const float4*>(L + c * kRT + 4);
    const float a[kRT] = {a0.x, a0.y, a0.z, a0.w, a1.x, a1.y, a1.z, a1.w};
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const float wj = lv[j] ? wq[j] : 0.f;
#pragma unroll
      for (int r = 0; r < kRT; ++r) acc[j][r] = fmaf(wj, a[r], acc[j][r]);
    }
  }
  __syncthreads();   // the lo tile is dead: its space takes the sums of waves 1..3
  if (wv > 0) {
#pragma unroll
    for (int j = 0; j < 4; ++j)
#pragma unroll
      for (int r = 0; r < kRT; ++r) L[((wv - 1) * 32 + j * kRT + r) * 64 + lane] = acc[j][r];
  }
  __syncthreads();
  if (wv == 0) {
#pragma unroll
    for (int j = 0; j < 4; ++j)
#pragma unroll
      for (int r = 0; r < kRT; ++r) {
        float s = acc[j][r];
        for (int q = 0; q < 3; ++q) s += L[(q * 32 + j * kRT + r) * 64 + lane];
        if (m + j < M && r0 + r < R) P[((long)z * M + m + j) * R + r0 + r] = s;
      }
  }
}

// hi[n][ch][iy][ix] = act(sum over the taps of the pixel's parity and the splits of P + bias[ch])
__global__ __launch_bounds__(256) void wfae_c3s2_scatter_final_kernel(const float* __restrict__ P, const float* __restrict__ bias,
                                                                      float* __restrict__ y, float* __restrict__ t, Geo g, long R,
                                                                      int splits, int act) {
  const int HWhi = g.Hhi * g.Whi, M = g.Chi * 9;
  const long total = (long)g.N * g.Chi * HWhi;
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
    const int p = (int)(i % HWhi), ch = (int)((i / HWhi) % g.Chi);
    const long n = i / ((long)HWhi * g.Chi);
    const int iy = p / g.Whi, ix = p % g.Whi;
    float s = 0.f;
    for (int ky = 0; ky < 3; ++ky) {
      const int ty = iy + 1 - ky;
      if (ty < 0 || (ty & 1) || (ty >> 1) >= g.Hlo) continue;
      for (int kx = 0; kx < 3; ++kx) {
        const int tx = ix + 1 - kx;
        if (tx < 0 || (tx & 1) || (tx >> 1) >= g.Wlo) continue;
        const long at = (long)(ch * 9 + ky * 3 + kx) * R + n * (g.Hlo * g.Wlo) + (ty >> 1) * g.Wlo + (tx >> 1);
        for (int z = 0; z < splits; ++z) s += P[(long)z * M * R + at];
      }
    }
    if (bias) s += bias[ch];
    if (t) t[i] = s;
    y[i] = act ? silu_f(s) : s;
  }
}

// dw (or a partial slab) element (cl, m): dead taps are exact zeros, or left alone when accumulating
__device__ __forceinline__ void store_dw(float* __restrict__ dw, long at, int m, float v, int live, int accumulate) {
  if ((live >> (m % 9)) & 1) dw[at] = accumulate ? dw[at] + v : v;
  else if (!accumulate) dw[at] = 0.f;
}

// ---- weight gradient: blockIdx.y < cl tiles: dw[cl][m] over the rows of split z; blockIdx.y == cl tiles: the bias gradient
__global__ __launch_bounds__(kThreads) void wfae_c3s2_wgrad_kernel(const float* __restrict__ hi, const float* __restrict__ thi,
                                                                   const float* __restrict__ lo, const float* __restrict__ tlo,
                                                                   float* __restrict__ dw, float* __restrict__ part,
                                                                   float* __restrict__ dbias, Geo g, long R, long rows_per_split,
                                                                   int splits, int cl_tiles, int bias_on_hi, int accumulate,
                                                                   bool vec) {
  __shared__ __attribute__((aligned(16))) float A[kRT * kKC];
  __shared__ __attribute__((aligned(16))) float Lt[kClt * kRT];
  __shared__ int4 ri[kRT];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  if ((int)blockIdx.y == cl_tiles) {
    // bias gradient: one wavefront per channel, the sum over (n, pixel) in a fixed order
    if (!dbias || blockIdx.z != 0) return;
    const int C = bias_on_hi ? g.Chi : g.Clo, HW = bias_on_hi ? g.Hhi * g.Whi : g.Hlo * g.Wlo;
    const float* __restrict__ v = bias_on_hi ? hi : lo;
    const float* __restrict__ tv = bias_on_hi ? thi : tlo;
    const long cnt = (long)g.N * HW;
    for (int c = blockIdx.x * 4 + wv; c < C; c += gridDim.x * 4) {
      float s = 0.f;
      for (long i = lane; i < cnt; i += 64) s += src_val(v, tv, ((i / HW) * C + c) * HW + i % HW);
      s = wave_sum(s);
      if (lane == 0) dbias[c] = accumulate ? dbias[c] + s : s;
    }
    return;
  }
  const int M = g.Chi * 9, HWlo = g.Hlo * g.Wlo;
  const int m0 = blockIdx.x * kKC, cl0 = blockIdx.y * kClt, z = blockIdx.z;
  const int mt = m0 + threadIdx.x, tap_t = mt % 9, ch_t = mt / 9;   // this thread's im2col column
  const long rb = (long)z * rows_per_split, re = min(R, rb + rows_per_split);
  float acc[kClw][4];
#pragma unroll
  for (int i = 0; i < kClw; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[i][j] = 0.f;
  for (long r0 = rb; r0 < re; r0 += kRT) {
    __syncthreads();   // the previous tile's readers
    if (threadIdx.x < kRT) ri[threadIdx.x] = row_info(r0 + threadIdx.x < re ? r0 + threadIdx.x : R, R, g);
    {
      const int c = threadIdx.x / kRT, cl = cl0 + c;
      const long r = r0 + threadIdx.x % kRT;
      Lt[threadIdx.x] = (cl < g.Clo && r < re) ? src_val(lo, tlo, ((r / HWlo) * g.Clo + cl) * HWlo + r % HWlo) : 0.f;
    }
    __syncthreads();
    stage_im2col(A, ri, hi, thi, g, ch_t, tap_t / 3, tap_t % 3, mt < M);
    __syncthreads();
#pragma unroll
    for (int r = 0; r < kRT; ++r) {
      const float4 a = *reinterpret_cast<const float4*>(A + r * kKC + 4 * lane);
#pragma unroll
      for (int i = 0; i < kClw; ++i) {
        const float s = Lt[(wv * kClw + i) * kRT + r];
        acc[i][0] = fmaf(s, a.x, acc[i][0]);
        acc[i][1] = fmaf(s, a.y, acc[i][1]);
        acc[i][2] = fmaf(s, a.z, acc[i][2]);
        acc[i][3] = fmaf(s, a.w, acc[i][3]);
      }
    }
  }
  const int m = m0 + 4 * lane;
#pragma unroll
  for (int i = 0; i < kClw; ++i) {
    const int cl = cl0 + wv * kClw + i;
    if (cl >= g.Clo) continue;
    const long at = (long)cl * M + m;
    if (splits > 1) {
      float* __restrict__ pz = part + (long)z * g.Clo * M;
      if (vec && m + 3 < M) *reinterpret_cast<float4*>(pz + at) = make_float4(acc[i][0], acc[i][1], acc[i][2], acc[i][3]);
      else
        for (int j = 0; j < 4; ++j)
          if (m + j < M) pz[at + j] = acc[i][j];
    } else if (vec && m + 3 < M && !accumulate) {
      float o[4];
#pragma unroll
      for (int j = 0; j < 4; ++j) o[j] = ((g.live >> ((m + j) % 9)) & 1) ? acc[i][j] : 0.f;
      *reinterpret_cast<float4*>(dw + at) = make_float4(o[0], o[1], o[2], o[3]);
    } else {
      for (int j = 0; j < 4; ++j)
        if (m + j < M) store_dw(dw, at + j, m + j, acc[i][j], g.live, accumulate);
    }
  }
}

__global__ __launch_bounds__(256) void wfae_c3s2_wgrad_final_kernel(const float* __restrict__ part, float* __restrict__ dw,
                                                                    long total, int M, int splits, int live, int accumulate) {
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
    float s = 0.f;
    for (int z = 0; z < splits; ++z) s += part[(long)z * total + i];
    store_dw(dw, i, (int)(i % M), s, live, accumulate);
  }
}

// ---- host side
int c3s2_geo(const char* what, int N, int Chi, int Clo, int Hhi, int Whi, int Hlo, int Wlo, Geo* g) {
  WFAE_REQUIRE(N > 0 && Chi > 0 && Clo > 0 && Hhi > 0 && Whi > 0 && Hlo > 0 && Wlo > 0, WFAE_ERR_BAD_SHAPE,
               "%s: sizes must be positive (N=%d Chi=%d Clo=%d hi %dx%d lo %dx%d)", what, N, Chi, Clo, Hhi, Whi, Hlo, Wlo);
  WFAE_REQUIRE(Hlo == (Hhi - 1) / 2 + 1 && Wlo == (Whi - 1) / 2 + 1, WFAE_ERR_UNSUPPORTED,
               "%s: planes %dx%d and %dx%d do not belong together: a 3x3 stride-2 padding-1 convolution takes %dx%d to "
               "%dx%d (the transposed one gives 2 lo - 1 + output_padding, output_padding 0 or 1)",
               what, Hhi, Whi, Hlo, Wlo, Hhi, Whi, (Hhi - 1) / 2 + 1, (Whi - 1) / 2 + 1);
  const long lim = 2147483647L;
  WFAE_REQUIRE((long)N * Chi * Hhi * Whi <= lim && (long)N * Clo * Hlo * Wlo <= lim && (long)Chi * Clo * 9 <= lim &&
                   (long)N * Hlo * Wlo <= lim && Chi <= (1 << 24) && Clo <= (1 << 24),
               WFAE_ERR_BAD_SHAPE, "%s: a tensor of 2^31 elements or more", what);
  *g = Geo{N, Chi, Clo, Hhi, Whi, Hlo, Wlo, live_mask(Hhi, Whi, Hlo, Wlo)};
  return 0;
}

struct Plan {
  int splits;
  long per_split;   // K chunks (gather), cl (scatter), rows (wgrad) of one split
  size_t ws;        // bytes
};
inline long cdivl(long a, long b) { return (a + b - 1) / b; }

Plan plan_gather(const Geo& g) {
  const long R = (long)g.N * g.Hlo * g.Wlo, nch = cdivl((long)g.Chi * 9, kKC);
  const long base = cdivl(g.Clo, kClt) * cdivl(R, kRT);
  long s = cdivl(kTargetBlocks, base);
  if (s > nch) s = nch;
  const long per = cdivl(nch, s);
  s = cdivl(nch, per);
  return Plan{(int)s, per, (size_t)s * g.Clo * R * sizeof(float)};
}
Plan plan_scatter(const Geo& g) {
  const long R = (long)g.N * g.Hlo * g.Wlo;
  const long base = cdivl((long)g.Chi * 9, kKC) * cdivl(R, kRT);
  long s = cdivl(kTargetBlocks, base);
  if (s > cdivl(g.Clo, 4)) s = cdivl(g.Clo, 4);     // at least one cl per wavefront
  if (s < cdivl(g.Clo, kSCl)) s = cdivl(g.Clo, kSCl);
  const long per = cdivl(g.Clo, s);
  s = cdivl(g.Clo, per);
  return Plan{(int)s, per, (size_t)s * g.Chi * 9 * R * sizeof(float)};
}
Plan plan_wgrad(const Geo& g) {
  const long R = (long)g.N * g.Hlo * g.Wlo, tiles = cdivl(R, kRT);
  const long base = cdivl((long)g.Chi * 9, kKC) * cdivl(g.Clo, kClt);
  long s = cdivl(kTargetBlocks, base);
  if (s > tiles) s = tiles;
  if (s > 64) s = 64;
  const long per = cdivl(tiles, s) * kRT;
  s = cdivl(R, per);
  return Plan{(int)s, per, s > 1 ? (size_t)s * g.Clo * g.Chi * 9 * sizeof(float) : (size_t)0};
}

inline bool vec_ok(const Geo& g, const void* w) { return (g.Chi * 9) % 4 == 0 && ((uintptr_t)w & 15) == 0; }
inline int grid_z_ok(const char* what, long y, long z) {
  WFAE_REQUIRE(y <= 65535 && z <= 65535, WFAE_ERR_UNSUPPORTED, "%s: %ld row tiles x %ld splits exceed the grid", what, y, z);
  return 0;
}

int run_gather(const char* what, const float* hi, const float* thi, const float* w, const float* bias, float* y, float* t,
               int act, const Geo& g, void* ws, size_t ws_bytes, hipStream_t st) {
  const Plan p = plan_gather(g);
  WFAE_REQUIRE(ws && ws_bytes >= p.ws, WFAE_ERR_WORKSPACE, "%s: workspace too small (%zu < %zu)", what, ws_bytes, p.ws);
  const long R = (long)g.N * g.Hlo * g.Wlo;
  int rc = grid_z_ok(what, cdivl(R, kRT), p.splits);
  if (rc) return rc;
  hipLaunchKernelGGL(wfae_c3s2_gather_kernel, dim3(cdivl(g.Clo, kClt), cdivl(R, kRT), p.splits), dim3(kThreads), 0, st, hi,
                     thi, w, (float*)ws, g, R, (int)p.per_split, vec_ok(g, w));
  if ((rc = check_launch(what))) return rc;
  hipLaunchKernelGGL(wfae_c3s2_gather_final_kernel, dim3(grid_1d((long)g.Clo * R, 1)), dim3(256), 0, st, (const float*)ws, bias,
                     y, t, g.Clo, R, g.Hlo * g.Wlo, p.splits, act);
  return check_launch(what);
}

int run_scatter(const char* what, const float* lo, const float* tlo, const float* w, const float* bias, float* y, float* t,
                int act, const Geo& g, void* ws, size_t ws_bytes, hipStream_t st) {
  const Plan p = plan_scatter(g);
  WFAE_REQUIRE(ws && ws_bytes >= p.ws, WFAE_ERR_WORKSPACE, "%s: workspace too small (%zu < %zu)", what, ws_bytes, p.ws);
  const long R = (long)g.N * g.Hlo * g.Wlo;
  int rc = grid_z_ok(what, cdivl(R, kRT), p.splits);
  if (rc) return rc;
  hipLaunchKernelGGL(wfae_c3s2_scatter_kernel, dim3(cdivl((long)g.Chi * 9, kKC), cdivl(R, kRT), p.splits), dim3(kThreads), 0, st,
                     lo, tlo, w, (float*)ws, g, R, (int)p.per_split, vec_ok(g, w));
  if ((rc = check_launch(what))) return rc;
  hipLaunchKernelGGL(wfae_c3s2_scatter_final_kernel, dim3(grid_1d((long)g.N * g.Chi * g.Hhi * g.Whi, 1)), dim3(256), 0, st,
                     (const float*)ws, bias, y, t, g, R, p.splits, act);
  return check_launch(what);
}

}  // namespace

extern "C" {

int wfae_c3s2_live_taps(int Hhi, int Whi, int Hlo, int Wlo) {
  WFAE_REQUIRE(Hhi > 0 && Whi > 0 && Hlo > 0 && Wlo > 0, WFAE_ERR_BAD_SHAPE, "c3s2_live_taps: sizes must be positive");
  WFAE_REQUIRE(Hlo == (Hhi - 1) / 2 + 1 && Wlo == (Whi - 1) / 2 + 1, WFAE_ERR_UNSUPPORTED,
               "c3s2_live_taps: planes %dx%d and %dx%d do not belong together", Hhi, Whi, Hlo, Wlo);
  return live_mask(Hhi, Whi, Hlo, Wlo);
}

size_t wfae_c3s2_workspace_bytes(int op, int transposed, int N, int Chi, int Clo, int Hhi, int Whi, int Hlo, int Wlo) {
  Geo g;
  if (op < 0 || op > 2 || c3s2_geo("c3s2_workspace_bytes", N, Chi, Clo, Hhi, Whi, Hlo, Wlo, &g)) return 0;
  if (op == 2) return plan_wgrad(g).ws;
  const bool gather = (op == 0) == (transposed == 0);   // forward of Conv2d, data gradient of ConvTranspose2d
  return gather ? plan_gather(g).ws : plan_scatter(g).ws;
}

int wfae_c3s2_fwd(const float* x, const float* w, const float* bias, float* y, float* t, int transposed, int act, int N,
                  int Chi, int Clo, int Hhi, int Whi, int Hlo, int Wlo, void* ws, size_t ws_bytes, wfae_stream_t stream) {
  WFAE_REQUIRE(x && w && y, WFAE_ERR_NULL_POINTER, "c3s2_fwd: null pointer");
  WFAE_REQUIRE(act == 0 || act == 1, WFAE_ERR_BAD_SHAPE, "c3s2_fwd: act %d (0 = none, 1 = SiLU)", act);
  Geo g;
  int rc = c3s2_geo("c3s2_fwd", N, Chi, Clo, Hhi, Whi, Hlo, Wlo, &g);
  if (rc) return rc;
  hipStream_t st = (hipStream_t)stream;
  return transposed ? run_scatter("c3s2_fwd", x, nullptr, w, bias, y, t, act, g, ws, ws_bytes, st)
                    : run_gather("c3s2_fwd", x, nullptr, w, bias, y, t, act, g, ws, ws_bytes, st);
}

int wfae_c3s2_bwd_data(const float* da, const float* t, const float* w, float* dx, int transposed, int act, int N, int Chi,
                       int Clo, int Hhi, int Whi, int Hlo, int Wlo, void* ws, size_t ws_bytes, wfae_stream_t stream) {
  WFAE_REQUIRE(da && w && dx && (t || act == 0), WFAE_ERR_NULL_POINTER, "c3s2_bwd_data: null pointer");
  WFAE_REQUIRE(act == 0 || act == 1, WFAE_ERR_BAD_SHAPE, "c3s2_bwd_data: act %d (0 = none, 1 = SiLU)", act);
  Geo g;
  int rc = c3s2_geo("c3s2_bwd_data", N, Chi, Clo, Hhi, Whi, Hlo, Wlo, &g);
  if (rc) return rc;
  hipStream_t st = (hipStream_t)stream;
  const float* tt = act ? t : nullptr;
  return transposed ? run_gather("c3s2_bwd_data", da, tt, w, nullptr, dx, nullptr, 0, g, ws, ws_bytes, st)
                    : run_scatter("c3s2_bwd_data", da, tt, w, nullptr, dx, nullptr, 0, g, ws, ws_bytes, st);
}

int wfae_c3s2_bwd_weight(const float* da, const float* t, const float* x, float* dw, float* dbias, int transposed, int act,
                         int accumulate, int N, int Chi, int Clo, int Hhi, int Whi, int Hlo, int Wlo, void* ws,
                         size_t ws_bytes, wfae_stream_t stream) {
  WFAE_REQUIRE(da && x && dw && (t || act == 0), WFAE_ERR_NULL_POINTER, "c3s2_bwd_weight: null pointer");
  WFAE_REQUIRE(act == 0 || act == 1, WFAE_ERR_BAD_SHAPE, "c3s2_bwd_weight: act %d (0 = none, 1 = SiLU)", act);
  Geo g;
  int rc = c3s2_geo("c3s2_bwd_weight", N, Chi, Clo, Hhi, Whi, Hlo, Wlo, &g);
  if (rc) return rc;
  const Plan p = plan_wgrad(g);
  WFAE_REQUIRE(p.ws == 0 || (ws && ws_bytes >= p.ws), WFAE_ERR_WORKSPACE, "c3s2_bwd_weight: workspace too small (%zu < %zu)",
               ws_bytes, p.ws);
  hipStream_t st = (hipStream_t)stream;
  const float* tt = act ? t : nullptr;
  // Conv2d: da, t live on the lo side and x on the hi side; ConvTranspose2d: the other way round
  const float *hi = transposed ? da : x, *thi = transposed ? tt : nullptr;
  const float *lo = transposed ? x : da, *tlo = transposed ? nullptr : tt;
  const long R = (long)g.N * g.Hlo * g.Wlo;
  const int cl_tiles = (int)cdivl(g.Clo, kClt);
  if ((rc = grid_z_ok("c3s2_bwd_weight", cl_tiles + 1, p.splits))) return rc;
  hipLaunchKernelGGL(wfae_c3s2_wgrad_kernel, dim3(cdivl((long)g.Chi * 9, kKC), cl_tiles + 1, p.splits), dim3(kThreads), 0, st,
                     hi, thi, lo, tlo, dw, (float*)ws, dbias, g, R, p.per_split, p.splits, cl_tiles, transposed ? 1 : 0,
                     accumulate ? 1 : 0, vec_ok(g, dw) && vec_ok(g, ws));
  if ((rc = check_launch("c3s2_bwd_weight"))) return rc;
  if (p.splits > 1) {
    hipLaunchKernelGGL(wfae_c3s2_wgrad_final_kernel, dim3(grid_1d((long)g.Clo * g.Chi * 9, 1)), dim3(256), 0, st,
                       (const float*)ws, dw, (long)g.Clo * g.Chi * 9, g.Chi * 9, p.splits, g.live, accumulate ? 1 : 0);
    rc = check_launch("c3s2_bwd_weight");
  }
  return rc;
}

}  // extern "C"
