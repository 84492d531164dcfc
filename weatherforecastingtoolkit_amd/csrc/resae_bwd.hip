// resae_bwd.hip — backward kernels of the ae_gan residual autoencoders (reference experiments/v1_experiments/ae_gan/train.py
// `ResidualBlock`, `UpsampleBlock`): the data and the weight gradient of the five layer kinds of resae.hip, and the join
// that ends a train-mode block,  y = gelu(c2 s2[c] + h2[c] + r),  forward and backward.
// NCHW fp32 in and out, the fp32 matrix instruction (v_mfma_f32_16x16x4_f32) with fp32 accumulation, a fixed summation
// order and no atomics: two launches give the same bits.
//
// Both gradients are GEMMs whose long dimension is a list of COLUMNS, one per pixel, taken 64 at a time (a column group).
//   route 1, "small": the columns are the pixels (n, y, x) of ALL samples in that order, so a group crosses samples; the
//     source pixels a group reads are the whole planes of the samples it touches.  For layers whose output plane has at
//     most 16 pixels, where one sample alone cannot fill a group.
//   route 0, "tile": a group is an 8 x 8 tile of one sample and its source pixels are the patch under the tile.  Any shape.
// The source pixels of a group are gathered into LDS once per 32 channels; a tap is an offset to an LDS record, or a
// literal zero where it is padding for that column.  DEAD taps (wfae_resae_live_taps) are skipped.
//
// Data gradient: columns = the pixels of dx (of the x2 grid for kind 2), K = Cout, the operand is the weight with in and
//   out channels transposed in the fragment order of the MFMA, read from HBM once per workgroup; the tap keeps its forward
//   index and the geometry runs backwards (dy row = (iy + 1 - ky) / S where that is exact and in range), which is the
//   180-degree rotation.  A workgroup owns 64 input channels x one group x a share of K; where K is split (small route) the
//   partial sums go to the workspace and a second launch adds them in ascending order.  Kind 2 sums each 2 x 2 block of
//   the x2 grid: in registers on the tile route, in the finishing launch on the small route.
// Weight gradient: K = the columns (the pixels of dy), a workgroup owns 64 output x 32 input channels for all nine taps and
//   a share of the groups; it writes each (co, ci)'s taps as one run, dead taps as zeros.  Where the groups are split
//   over workgroups the partial dw go to the workspace and are added in ascending order.
#include "common.h"
#include "resae_common.h"

using namespace wfae;
using namespace wfae::resae_geo;

namespace {

typedef float f32x4 __attribute__((ext_vector_type(4)));

constexpr int CK = 32;            // channels per LDS chunk
constexpr int kThreads = 256;
constexpr int SCG = 64;           // columns of a group
constexpr int TS = 8;             // side of a tile-route group
constexpr int SREC = CK + 4;      // floats of one LDS pixel record
constexpr int DST = SCG + 4;      // floats of one dy row of the weight gradient in LDS
constexpr int kSmallMaxPlane = 16;
constexpr int kTargetWgs = 512;
constexpr int kMaxGroupsPerSplit = 64;
constexpr size_t kLdsLimit = 128 * 1024;

enum { DIR_FWD = 0, DIR_BWD = 1 };   // the columns are output pixels and read the input (weight gradient) / the reverse

// how the groups of 64 columns map to pixels and which source pixels a group stages
struct CG {
  int route, dir, kind;
  int N, GH, GW;       // the column grid
  int SH, SW;          // the source plane
  int PH, PW;          // source pixels staged per sample: the whole plane (small) or the patch under a tile
  int tx, ty;          // tiles per sample (tile route)
  int pnum, pden, poff;   // patch origin of a tile at c0: c0 * pnum / pden + poff
  int R;               // N GH GW
  int groups;
};

struct Grp {
  int n0, ns, py0, px0, cy0, cx0, col0;
};

__device__ __forceinline__ Grp group_of(const CG& g, int gi) {
  Grp q;
  if (g.route == 1) {
    const int P = g.GH * g.GW;
    q.col0 = gi * SCG;
    q.n0 = q.col0 / P;
    const int n1 = min(g.N - 1, (q.col0 + SCG - 1) / P);
    q.ns = n1 - q.n0 + 1;
    q.py0 = q.px0 = q.cy0 = q.cx0 = 0;
  } else {
    const int per = g.tx * g.ty, t = gi % per;
    q.col0 = 0;
    q.n0 = gi / per;
    q.ns = 1;
    q.cy0 = (t / g.tx) * TS;
    q.cx0 = (t % g.tx) * TS;
    q.py0 = q.cy0 * g.pnum / g.pden + g.poff;
    q.px0 = q.cx0 * g.pnum / g.pden + g.poff;
  }
  return q;
}

// column c (0..63) of the group -> its pixel; false where the group has no such column
__device__ __forceinline__ bool column_of(const CG& g, const Grp& q, int c, int& n, int& cy, int& cx) {
  if (g.route == 1) {
    const int col = q.col0 + c, P = g.GH * g.GW;
    if (col >= g.R) return false;
    n = col / P;
    const int o = col - n * P;
    cy = o / g.GW;
    cx = o - cy * g.GW;
    return true;
  }
  n = q.n0;
  cy = q.cy0 + c / TS;
  cx = q.cx0 + c % TS;
  return cy < g.GH && cx < g.GW;
}

// source index along one axis of column position i through tap k, or -1: the forward rule, or its inverse
__device__ __forceinline__ int src_of(int dir, int kind, int i, int k, int sh) {
  if (kind_taps(kind) == 1 && k != 1) return -1;
  if (dir == DIR_FWD) return src_index(kind, i, k, sh);   // sh: the input plane
  // backward: the dy position o with  S o + k - 1 == i  (kind 2: on the x2 grid, S = 1); sh: the dy plane
  const int t = i + 1 - k;
  if (t < 0) return -1;
  if (kind_stride(kind) == 2) {
    if (t & 1) return -1;
    return (t >> 1) < sh ? (t >> 1) : -1;
  }
  return t < sh ? t : -1;
}

// LDS record (in floats) of source pixel (n, sy, sx) of the group, or -1
__device__ __forceinline__ int record_of(const CG& g, const Grp& q, int n, int cy, int cx, int tap) {
  const int sy = src_of(g.dir, g.kind, cy, tap / 3, g.SH), sx = src_of(g.dir, g.kind, cx, tap % 3, g.SW);
  if (sy < 0 || sx < 0) return -1;
  const int py = sy - q.py0, px = sx - q.px0;
  if (py < 0 || py >= g.PH || px < 0 || px >= g.PW) return -1;   // never taken: the patch covers every tap of the group
  return (((n - q.n0) * g.PH + py) * g.PW + px) * SREC;
}

// gather channels c0 .. c0 + 31 of the group's source pixels: item = (record, 4 channels), lanes run along the records
__device__ __forceinline__ void stage_source(const CG& g, const Grp& q, const float* __restrict__ src, int C, int c0, float* xs, int t) {
  const int PP = g.PH * g.PW, nrec = q.ns * PP;
  const long plane = (long)g.SH * g.SW;
  for (int it = t; it < nrec * 8; it += kThreads) {
    const int rec = it % nrec, gq = it / nrec;
    const int nr = rec / PP, pp = rec - nr * PP;
    const int py = pp / g.PW, px = pp - py * g.PW;
    const int sy = q.py0 + py, sx = q.px0 + px;
    const bool ok = sy >= 0 && sy < g.SH && sx >= 0 && sx < g.SW;
    const float* __restrict__ p = src + ((long)(q.n0 + nr) * C) * plane + (ok ? sy * g.SW + sx : 0);
    const int c = c0 + 4 * gq;
    f32x4 v;
#pragma unroll
    for (int j = 0; j < 4; ++j) v[j] = (ok && c + j < C) ? p[(long)(c + j) * plane] : 0.f;
    *reinterpret_cast<f32x4*>(xs + rec * SREC + 4 * gq) = v;
  }
}

// ---------------------------------------------------------------------------------------------------- data gradient
struct DP {
  const float* dy;
  const float* w;     // packed_t
  const float* add;
  float* dx;
  float* ws;
  CG g;
  int Cin, Cout, H, W, ncib, nkb, nchunks, per_split, live, out_mode;
};
enum { OUT_WS = 0, OUT_DIRECT = 1, OUT_UPSUM = 2 };

// packed_t[tap < T][cib][kb][lane = 16 g4 + r15][c < 4] = w[co = 16 kb + 4 g4 + c][ci = 16 cib + r15][tap]
__global__ __launch_bounds__(256) void resae_bwd_pack_kernel(const float* __restrict__ w, float* __restrict__ out, int Cout, int Cin,
                                                             int ncib, int nkb, int T) {
  // one thread per (co, ci): it reads the T taps of the pair, one run of the raw weight, and writes one float per tap plane;
  // the 16 ci of a lane group are neighbours in w, the threads of a wave neighbours in every plane
  const long plane = (long)ncib * nkb * 256;
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= plane) return;
  const int c = (int)(i & 3), lane = (int)((i >> 2) & 63);
  const long r = i >> 8;
  const int kb = (int)(r % nkb), cib = (int)(r / nkb);
  const int ci = 16 * cib + (lane & 15), co = 16 * kb + 4 * (lane >> 4) + c;
  const bool ok = co < Cout && ci < Cin;
  const float* __restrict__ p = w + ((long)co * Cin + ci) * T;
  for (int tap = 0; tap < T; ++tap) out[tap * plane + i] = ok ? p[tap] : 0.f;
}

__global__ __launch_bounds__(kThreads) void resae_bwd_data_kernel(DP p) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  float* xs = reinterpret_cast<float*>(smem);
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6, r15 = lane & 15, g4 = lane >> 4;
  const int cib = blockIdx.y * 4 + wave;
  const bool wave_on = cib < p.ncib;
  const int T = kind_taps(p.g.kind);
  const Grp q = group_of(p.g, blockIdx.x);
  const int cc0 = blockIdx.z * p.per_split, cc1 = min(p.nchunks, cc0 + p.per_split);

  // this lane's four columns (one per 16-column tile) and, per tap, the LDS record they read or -1 for a literal zero
  int cn[4], cy[4], cx[4], off[4][9];
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    int n = 0, y = 0, x = 0;
    const bool cv = column_of(p.g, q, 16 * j + r15, n, y, x);
    cn[j] = cv ? n : -1;
    cy[j] = y;
    cx[j] = x;
#pragma unroll
    for (int tap = 0; tap < 9; ++tap) off[j][tap] = cv ? record_of(p.g, q, n, y, x, tap) : -1;
  }

  f32x4 acc[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) acc[j] = f32x4{0.f, 0.f, 0.f, 0.f};

  for (int cc = cc0; cc < cc1; ++cc) {
    f32x4 a[9][2];
#pragma unroll
    for (int tap = 0; tap < 9; ++tap)
#pragma unroll
      for (int hf = 0; hf < 2; ++hf) {
        a[tap][hf] = f32x4{0.f, 0.f, 0.f, 0.f};
        if (wave_on && ((p.live >> tap) & 1)) {
          const int ts = T == 9 ? tap : 0;
          a[tap][hf] = *reinterpret_cast<const f32x4*>(p.w + ((((long)ts * p.ncib + cib) * p.nkb + 2 * cc + hf) * 64 + lane) * 4);
        }
      }
    __syncthreads();   // the fragment reads of the previous chunk are done
    stage_source(p.g, q, p.dy, p.Cout, cc * CK, xs, t);
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
  // accumulator register r of lane (r15, g4) is (ci = 16 cib + 4 g4 + r, column 16 j + r15 of the group)
  const long HW = (long)p.H * p.W;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int ci = 16 * cib + 4 * g4 + r;
      float v = acc[j][r];
      if (p.out_mode == OUT_UPSUM) {
        // tile route, kind 2: column 16 j + r15 is pixel (2 j + (r15 >> 3), r15 & 7) of the tile; its 2 x 2 block mates are
        // lanes r15 ^ 1 and r15 ^ 8.  Columns outside the grid hold zeros.  All lanes of the wave take part.
        v += __shfl_xor(v, 1, 64);
        v += __shfl_xor(v, 8, 64);
        if (cn[j] >= 0 && ci < p.Cin && !(cy[j] & 1) && !(cx[j] & 1)) {
          const long o = ((long)cn[j] * p.Cin + ci) * HW + (long)(cy[j] >> 1) * p.W + (cx[j] >> 1);
          p.dx[o] = p.add ? v + p.add[o] : v;
        }
      } else if (cn[j] >= 0) {
        if (p.out_mode == OUT_DIRECT) {
          if (ci < p.Cin) {
            const long o = ((long)cn[j] * p.Cin + ci) * HW + (long)cy[j] * p.W + cx[j];
            p.dx[o] = p.add ? v + p.add[o] : v;
          }
        } else {
          const long pid = ((long)cn[j] * p.g.GH + cy[j]) * p.g.GW + cx[j];
          p.ws[((long)blockIdx.z * p.ncib * 16 + ci) * p.g.R + pid] = v;
        }
      }
    }
  }
}

// the partial sums of the K splits added in ascending split order (kind 2: the four pixels of a 2 x 2 block in row-major
// order, each over its splits), then `add`; one thread per element of dx
__global__ __launch_bounds__(256) void resae_bwd_data_final_kernel(const float* __restrict__ ws, const float* __restrict__ add,
                                                                   float* __restrict__ dx, int N, int Cin, int H, int W, int up, int rows,
                                                                   int splits) {
  const long HW = (long)H * W, per_c = (long)N * HW;
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= per_c * Cin) return;
  const int ci = (int)(i / per_c);
  const long rem = i - ci * per_c;
  const int n = (int)(rem / HW), ip = (int)(rem - n * HW), iy = ip / W, ix = ip - iy * W;
  const int f = up ? 2 : 1, GH = f * H, GW = f * W;
  const long R = (long)N * GH * GW;
  float v = 0.f;
  for (int a = 0; a < f; ++a)
    for (int b = 0; b < f; ++b) {
      const long pid = ((long)n * GH + f * iy + a) * GW + f * ix + b;
      float s = 0.f;
      for (int k = 0; k < splits; ++k) s += ws[((long)k * rows + ci) * R + pid];
      v += s;
    }
  const long o = ((long)n * Cin + ci) * HW + ip;
  dx[o] = add ? v + add[o] : v;
}

// -------------------------------------------------------------------------------------------------- weight gradient
struct WP {
  const float* dy;
  const float* x;
  float* out;   // dw, or the workspace where the groups are split
  CG g;
  int Cin, Cout, Ho, Wo, T, per_split, live;
  long slab;    // floats of one partial dw
};

__global__ __launch_bounds__(kThreads) void resae_bwd_weight_kernel(WP p) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  float* dys = reinterpret_cast<float*>(smem);            // [64 co][DST]
  int* offs = reinterpret_cast<int*>(dys + 64 * DST);     // [9 taps][64 columns]
  float* xs = reinterpret_cast<float*>(offs + 9 * SCG);   // [records][SREC]
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6, r15 = lane & 15, g4 = lane >> 4;
  const int ci0 = blockIdx.x * CK, co0 = blockIdx.y * 64;
  const int g0 = blockIdx.z * p.per_split, g1 = min(p.g.groups, g0 + p.per_split);
  const long HoWo = (long)p.Ho * p.Wo;

  f32x4 acc[9][2];
#pragma unroll
  for (int tap = 0; tap < 9; ++tap)
#pragma unroll
    for (int h = 0; h < 2; ++h) acc[tap][h] = f32x4{0.f, 0.f, 0.f, 0.f};

  for (int gi = g0; gi < g1; ++gi) {
    const Grp q = group_of(p.g, gi);
    __syncthreads();   // the reads of the previous group are done
    stage_source(p.g, q, p.x, p.Cin, ci0, xs, t);
    {
      // thread t serves column t & 63 in every item it takes: dy of 16 output channels, and two or three taps' records
      const int c = t & 63;
      int n = 0, y = 0, x = 0;
      const bool cv = column_of(p.g, q, c, n, y, x);
      const float* __restrict__ dp = p.dy + ((long)n * p.Cout) * HoWo + (long)y * p.Wo + x;
      for (int col = wave; col < 64; col += 4) {
        const int co = co0 + col;
        dys[col * DST + c] = (cv && co < p.Cout) ? dp[(long)co * HoWo] : 0.f;
      }
      for (int tap = wave; tap < 9; tap += 4) offs[tap * SCG + c] = cv ? record_of(p.g, q, n, y, x, tap) : -1;
    }
    __syncthreads();
    const float* __restrict__ arow = dys + (16 * wave + r15) * DST + g4;
#pragma unroll 4
    for (int ks = 0; ks < SCG / 4; ++ks) {
      const float a = arow[4 * ks];
#pragma unroll
      for (int tap = 0; tap < 9; ++tap) {
        if (!((p.live >> tap) & 1)) continue;   // dead taps keep their zeros
        const int o = offs[tap * SCG + 4 * ks + g4];
        const float b0 = o >= 0 ? xs[o + r15] : 0.f;
        const float b1 = o >= 0 ? xs[o + 16 + r15] : 0.f;
        acc[tap][0] = __builtin_amdgcn_mfma_f32_16x16x4f32(a, b0, acc[tap][0], 0, 0, 0);
        acc[tap][1] = __builtin_amdgcn_mfma_f32_16x16x4f32(a, b1, acc[tap][1], 0, 0, 0);
      }
    }
  }
  // accumulator register r of lane (r15, g4) is (co = co0 + 16 wave + 4 g4 + r, ci = ci0 + 16 h + r15): nine taps = one run
  float* __restrict__ out = p.out + (long)blockIdx.z * p.slab;
#pragma unroll
  for (int h = 0; h < 2; ++h)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int co = co0 + 16 * wave + 4 * g4 + r, ci = ci0 + 16 * h + r15;
      if (co >= p.Cout || ci >= p.Cin) continue;
      float* __restrict__ o = out + ((long)co * p.Cin + ci) * p.T;
      if (p.T == 9) {
#pragma unroll
        for (int tap = 0; tap < 9; ++tap) o[tap] = acc[tap][h][r];
      } else {
        o[0] = acc[4][h][r];
      }
    }
}

// dw = the partial slabs added in ascending order
__global__ __launch_bounds__(256) void resae_bwd_weight_final_kernel(const float* __restrict__ ws, float* __restrict__ dw, long total, int splits) {
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= total) return;
  float v = 0.f;
  for (int s = 0; s < splits; ++s) v += ws[(long)s * total + i];
  dw[i] = v;
}

// dbias[co] = the sum of dy over (n, oy, ox): one workgroup per channel, strided partial sums, then a tree in LDS
__global__ __launch_bounds__(256) void resae_bwd_bias_kernel(const float* __restrict__ dy, float* __restrict__ dbias, int N, int Cout, long HoWo) {
  __shared__ float red[256];
  const int co = blockIdx.x, t = threadIdx.x;
  float v = 0.f;
  for (int n = 0; n < N; ++n) {
    const float* __restrict__ p = dy + ((long)n * Cout + co) * HoWo;
    for (long i = t; i < HoWo; i += 256) v += p[i];
  }
  red[t] = v;
  __syncthreads();
  for (int s = 128; s > 0; s >>= 1) {
    if (t < s) red[t] += red[t + s];
    __syncthreads();
  }
  if (t == 0) dbias[co] = red[0];
}

// ------------------------------------------------------------------------------------------------------------- join
struct JP {
  const float* c2;
  const float* s2;
  const float* h2;
  const float* r;
  const float* ss;
  const float* hs;
  const float* dy;
  float* y;      // forward
  float* dpre;   // backward
  float* dres;   // backward, res_mode 2
  int C, H, W, res_mode;
  long total;    // elements of y (res_mode 1) or of r (res_mode 2): one thread each
};

__device__ __forceinline__ float join_res(const JP& p, int c, long ri) {
  const float r = p.r[ri];
  return p.ss ? fmaf(r, p.ss[c], p.hs[c]) : r;
}

template <bool BWD>
__global__ __launch_bounds__(256) void resae_join_kernel(JP p) {
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= p.total) return;
  if (p.res_mode == 1) {
    const int c = (int)((i / ((long)p.H * p.W)) % p.C);
    const float pre = fmaf(p.c2[i], p.s2[c], p.h2[c]) + join_res(p, c, i);
    if (BWD) p.dpre[i] = p.dy[i] * gelu_grad_f(pre);
    else p.y[i] = gelu_f(pre);
    return;
  }
  // one thread per pixel of the half-resolution residual: its 2 x 2 block of y, in row-major order
  const int h2 = p.H >> 1, w2 = p.W >> 1;
  const long plane2 = (long)h2 * w2;
  const long nc = i / plane2;
  const int c = (int)(nc % p.C), ip = (int)(i - nc * plane2), ry = ip / w2, rx = ip - ry * w2;
  const float res = join_res(p, c, i);
  const float s = p.s2[c], h = p.h2[c];
  float sum = 0.f;
#pragma unroll
  for (int a = 0; a < 2; ++a)
#pragma unroll
    for (int b = 0; b < 2; ++b) {
      const long o = (nc * p.H + 2 * ry + a) * p.W + 2 * rx + b;
      const float pre = fmaf(p.c2[o], s, h) + res;
      if (BWD) {
        const float d = p.dy[o] * gelu_grad_f(pre);
        p.dpre[o] = d;
        sum += d;
      } else {
        p.y[o] = gelu_f(pre);
      }
    }
  if (BWD) p.dres[i] = sum;
}

// running statistics of a BatchNorm whose input is read through the x2 upsample (the shortcut of an UpsampleBlock): mean
// and biased variance are those of the source tensor, the unbiased factor counts every value `replicas` times
__global__ __launch_bounds__(128) void resae_bn_running_kernel(const float* __restrict__ mean, const float* __restrict__ invstd,
                                                               float* __restrict__ running_mean, float* __restrict__ running_var, int C,
                                                               float eps, float momentum, double count) {
  const int c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= C) return;
  const double is = (double)invstd[c];
  double var = 1.0 / (is * is) - (double)eps;
  if (var < 0.0) var = 0.0;
  const double unb = count > 1.0 ? var * (count / (count - 1.0)) : var;
  running_mean[c] = (1.f - momentum) * running_mean[c] + momentum * mean[c];
  running_var[c] = (1.f - momentum) * running_var[c] + momentum * (float)unb;
}

// ------------------------------------------------------------------------------------------------------------ plans
struct Plan {
  CG g;
  int splits, per_split, nchunks, out_mode;
  size_t ws, lds;
};

int check_layer(const char* what, int route, int kind, int N, int Cin, int Cout, int H, int W) {
  WFAE_REQUIRE(route == 0 || route == 1, WFAE_ERR_BAD_SHAPE, "%s: route %d (0 = tile, 1 = small)", what, route);
  WFAE_REQUIRE(kind >= K3S1 && kind <= K1S2, WFAE_ERR_BAD_SHAPE,
               "%s: kind %d (0 = 3x3 s1 p1, 1 = 3x3 s2 p1, 2 = x2 nearest upsample + 3x3 s1 p1, 3 = 1x1 s1, 4 = 1x1 s2)", what, kind);
  WFAE_REQUIRE(N > 0 && H > 0 && W > 0 && H <= 8192 && W <= 8192, WFAE_ERR_BAD_SHAPE, "%s: bad shape N=%d H=%d W=%d", what, N, H, W);
  WFAE_REQUIRE(Cout > 0 && Cin > 0 && Cout <= 4096 && Cin <= 4096, WFAE_ERR_UNSUPPORTED,
               "%s: channel counts 1..4096 are served (got Cout=%d Cin=%d)", what, Cout, Cin);
  const long Ho = out_size(kind, H), Wo = out_size(kind, W);
  WFAE_REQUIRE((long)Cin * H * W < (1l << 31) && (long)Cout * Ho * Wo < (1l << 31), WFAE_ERR_BAD_SHAPE,
               "%s: one sample must stay below 2^31 elements", what);
  WFAE_REQUIRE((long)N * Ho * Wo < (1l << 31) && (long)N * H * W < (1l << 31), WFAE_ERR_BAD_SHAPE,
               "%s: N times a plane must stay below 2^31 pixels", what);
  if (route == 1) {
    WFAE_REQUIRE(Ho * Wo <= kSmallMaxPlane, WFAE_ERR_UNSUPPORTED,
                 "%s: the small-plane route serves output planes of at most %d pixels (got %ldx%ld)", what, kSmallMaxPlane, Ho, Wo);
    WFAE_REQUIRE((long)N * Ho * Wo < (1l << 21) && (long)N * H * W < (1l << 21), WFAE_ERR_UNSUPPORTED,
                 "%s: the small-plane route serves N H W < 2^21", what);
  }
  return WFAE_OK;
}

// the column geometry both plans share; dir = DIR_BWD: columns on the dx grid reading dy, DIR_FWD: columns on the dy grid
// reading x
CG geometry(int route, int dir, int kind, int N, int H, int W) {
  CG g = {};
  const int Ho = out_size(kind, H), Wo = out_size(kind, W);
  g.route = route; g.dir = dir; g.kind = kind; g.N = N;
  if (dir == DIR_BWD) {
    g.GH = kind == K3UP ? 2 * H : H; g.GW = kind == K3UP ? 2 * W : W;
    g.SH = Ho; g.SW = Wo;
  } else {
    g.GH = Ho; g.GW = Wo;
    g.SH = H; g.SW = W;
  }
  g.R = N * g.GH * g.GW;
  if (route == 1) {
    g.PH = g.SH; g.PW = g.SW;
    g.tx = g.ty = 1; g.pnum = g.pden = 1; g.poff = 0;
    g.groups = cdiv(g.R, SCG);
    return g;
  }
  g.tx = cdiv(g.GW, TS); g.ty = cdiv(g.GH, TS);
  g.groups = N * g.tx * g.ty;
  // the source rows under a tile of 8 column rows that starts at c0 (a multiple of 8): first row and row count
  int ph;
  g.pnum = g.pden = 1; g.poff = 0;
  if (dir == DIR_BWD) {
    switch (kind) {
      case K3S1: case K3UP: g.poff = -1; ph = TS + 2; break;          // i + 1 - k
      case K3S2: g.pden = 2; ph = TS / 2 + 1; break;                   // (i + 1 - k) / 2 where even: c0 / 2 .. c0 / 2 + 4
      case K1S1: ph = TS; break;
      default: g.pden = 2; ph = TS / 2; break;                         // i / 2 where even
    }
  } else {
    switch (kind) {
      case K3S1: g.poff = -1; ph = TS + 2; break;                      // o + k - 1
      case K3S2: g.pnum = 2; g.poff = -1; ph = 2 * (TS - 1) + 3; break;   // 2 o + k - 1
      case K3UP: g.pden = 2; g.poff = -1; ph = TS / 2 + 2; break;      // (o + k - 1) >> 1: c0 / 2 - 1 .. c0 / 2 + 4
      case K1S1: ph = TS; break;
      default: g.pnum = 2; ph = 2 * (TS - 1) + 1; break;               // 2 o
    }
  }
  g.PH = g.PW = ph;
  return g;
}

// samples a small-route group can touch
inline int group_samples(const CG& g) {
  const int cap = (SCG - 1) / (g.GH * g.GW) + 2;
  return g.N < cap ? g.N : cap;
}

Plan plan_data(int route, int kind, int N, int Cin, int Cout, int H, int W) {
  Plan q = {};
  q.g = geometry(route, DIR_BWD, kind, N, H, W);
  q.nchunks = cdiv(Cout, CK);
  const int ncib = cdiv(Cin, 16), slabs = cdiv(ncib, 4);
  if (route == 1) {
    int splits = cdiv(kTargetWgs, (int64_t)slabs * q.g.groups);
    splits = splits < 1 ? 1 : splits > q.nchunks ? q.nchunks : splits;
    q.per_split = cdiv(q.nchunks, splits);
    q.splits = cdiv(q.nchunks, q.per_split);
    q.out_mode = (q.splits == 1 && kind != K3UP) ? OUT_DIRECT : OUT_WS;
    q.ws = q.out_mode == OUT_WS ? (size_t)q.splits * ncib * 16 * q.g.R * sizeof(float) : 0;
    q.lds = (size_t)group_samples(q.g) * q.g.PH * q.g.PW * SREC * sizeof(float);
  } else {
    q.splits = 1;
    q.per_split = q.nchunks;
    q.out_mode = kind == K3UP ? OUT_UPSUM : OUT_DIRECT;
    q.lds = (size_t)q.g.PH * q.g.PW * SREC * sizeof(float);
  }
  return q;
}

Plan plan_weight(int route, int kind, int N, int Cin, int Cout, int H, int W) {
  Plan q = {};
  q.g = geometry(route, DIR_FWD, kind, N, H, W);
  const int64_t tiles = (int64_t)cdiv(Cin, CK) * cdiv(Cout, 64);
  int splits = cdiv(kTargetWgs, tiles);
  const int least = cdiv(q.g.groups, kMaxGroupsPerSplit);
  splits = splits < least ? least : splits;
  splits = splits > q.g.groups ? q.g.groups : splits;
  q.per_split = cdiv(q.g.groups, splits);
  q.splits = cdiv(q.g.groups, q.per_split);
  q.ws = q.splits > 1 ? (size_t)q.splits * Cout * Cin * kind_taps(kind) * sizeof(float) : 0;
  const size_t rec = (size_t)(route == 1 ? group_samples(q.g) : 1) * q.g.PH * q.g.PW;
  q.lds = (64 * DST + 9 * SCG + rec * SREC) * sizeof(float);
  return q;
}

int check_ws(const char* what, const Plan& q, const void* ws, size_t ws_bytes) {
  WFAE_REQUIRE(q.lds <= kLdsLimit, WFAE_ERR_UNSUPPORTED, "%s: this shape needs %zu bytes of LDS on this route", what, q.lds);
  WFAE_REQUIRE(q.ws == 0 || (ws && ws_bytes >= q.ws), WFAE_ERR_WORKSPACE, "%s: workspace too small (%zu < %zu)", what, ws_bytes, q.ws);
  WFAE_REQUIRE(q.ws == 0 || (reinterpret_cast<uintptr_t>(ws) & 3) == 0, WFAE_ERR_WORKSPACE, "%s: workspace must be 4-byte aligned", what);
  return WFAE_OK;
}

int check_join(const char* what, int res_mode, int N, int C, int H, int W, bool affine_pair_ok) {
  WFAE_REQUIRE(res_mode == 1 || res_mode == 2, WFAE_ERR_BAD_SHAPE,
               "%s: res_mode %d (1 = the residual at y's resolution, 2 = at half resolution, read through a x2 nearest upsample)", what, res_mode);
  WFAE_REQUIRE(affine_pair_ok, WFAE_ERR_BAD_SHAPE, "%s: ss and hs go together (both, or neither for the identity shortcut)", what);
  WFAE_REQUIRE(N > 0 && C > 0 && H > 0 && W > 0 && H <= 8192 && W <= 8192, WFAE_ERR_BAD_SHAPE, "%s: bad shape N=%d C=%d H=%d W=%d", what, N, C, H, W);
  WFAE_REQUIRE(res_mode != 2 || (H % 2 == 0 && W % 2 == 0), WFAE_ERR_BAD_SHAPE,
               "%s: a residual read through the upsample needs an even plane (got %dx%d)", what, H, W);
  WFAE_REQUIRE((long)N * C * H * W < (1l << 38), WFAE_ERR_BAD_SHAPE, "%s: tensor too large", what);
  return WFAE_OK;
}

template <bool BWD>
int launch_join(JP p, int N, hipStream_t st, const char* what) {
  const long plane = p.res_mode == 2 ? (long)(p.H >> 1) * (p.W >> 1) : (long)p.H * p.W;
  p.total = (long)N * p.C * plane;
  hipLaunchKernelGGL(resae_join_kernel<BWD>, dim3((unsigned)((p.total + 255) / 256)), dim3(256), 0, st, p);
  return check_launch(what);
}

}  // namespace

extern "C" {

size_t wfae_resae_bwd_pack_bytes(int kind, int Cout, int Cin) {
  if (kind < K3S1 || kind > K1S2 || Cout <= 0 || Cin <= 0 || Cout > 4096 || Cin > 4096) return 0;
  return (size_t)kind_taps(kind) * cdiv(Cin, 16) * 2 * cdiv(Cout, CK) * 256 * sizeof(float);
}

int wfae_resae_bwd_pack(const float* w, void* packed_t, int kind, int Cout, int Cin, wfae_stream_t stream) {
  WFAE_REQUIRE(w && packed_t, WFAE_ERR_NULL_POINTER, "resae_bwd_pack: null pointer");
  WFAE_REQUIRE(kind >= K3S1 && kind <= K1S2, WFAE_ERR_BAD_SHAPE, "resae_bwd_pack: kind %d, expected 0..4", kind);
  WFAE_REQUIRE(Cout > 0 && Cin > 0 && Cout <= 4096 && Cin <= 4096, WFAE_ERR_UNSUPPORTED,
               "resae_bwd_pack: channel counts 1..4096 are served (got Cout=%d Cin=%d)", Cout, Cin);
  WFAE_REQUIRE((reinterpret_cast<uintptr_t>(packed_t) & 15) == 0, WFAE_ERR_BAD_SHAPE, "resae_bwd_pack: packed_t must be 16-byte aligned");
  const int T = kind_taps(kind), ncib = cdiv(Cin, 16), nkb = 2 * cdiv(Cout, CK);
  const long plane = (long)ncib * nkb * 256;   // one thread per element of a tap plane
  hipLaunchKernelGGL(resae_bwd_pack_kernel, dim3((unsigned)((plane + 255) / 256)), dim3(256), 0, (hipStream_t)stream, w, (float*)packed_t,
                     Cout, Cin, ncib, nkb, T);
  return check_launch("resae_bwd_pack");
}

size_t wfae_resae_bwd_data_workspace_bytes(int route, int kind, int N, int Cin, int Cout, int H, int W) {
  if (check_layer("resae_bwd_data_workspace_bytes", route, kind, N, Cin, Cout, H, W)) return 0;
  return plan_data(route, kind, N, Cin, Cout, H, W).ws;
}

int wfae_resae_bwd_data(const float* dy, const void* packed_t, const float* add, float* dx, int route, int kind, int N, int Cin,
                        int Cout, int H, int W, void* ws, size_t ws_bytes, wfae_stream_t stream) {
  WFAE_REQUIRE(dy && packed_t && dx, WFAE_ERR_NULL_POINTER, "resae_bwd_data: null pointer");
  int rc = check_layer("resae_bwd_data", route, kind, N, Cin, Cout, H, W);
  if (rc) return rc;
  WFAE_REQUIRE((reinterpret_cast<uintptr_t>(packed_t) & 15) == 0, WFAE_ERR_BAD_SHAPE, "resae_bwd_data: packed_t must be 16-byte aligned");
  const Plan q = plan_data(route, kind, N, Cin, Cout, H, W);
  if ((rc = check_ws("resae_bwd_data", q, ws, ws_bytes))) return rc;
  const int ncib = cdiv(Cin, 16), slabs = cdiv(ncib, 4);
  WFAE_REQUIRE(slabs <= 65535 && q.splits <= 65535, WFAE_ERR_BAD_SHAPE, "resae_bwd_data: grid too large");
  DP p = {};
  p.dy = dy; p.w = (const float*)packed_t; p.add = add; p.dx = dx; p.ws = (float*)ws; p.g = q.g;
  p.Cin = Cin; p.Cout = Cout; p.H = H; p.W = W; p.ncib = ncib; p.nkb = 2 * q.nchunks; p.nchunks = q.nchunks;
  p.per_split = q.per_split; p.live = live_mask(kind, H, W); p.out_mode = q.out_mode;
  hipStream_t st = (hipStream_t)stream;
  (void)hipFuncSetAttribute((const void*)resae_bwd_data_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)kLdsLimit);
  hipLaunchKernelGGL(resae_bwd_data_kernel, dim3(q.g.groups, slabs, q.splits), dim3(kThreads), q.lds, st, p);
  if ((rc = check_launch("resae_bwd_data"))) return rc;
  if (q.out_mode == OUT_WS) {
    const long total = (long)N * Cin * H * W;   // one thread per element, below 2^33: at most 2^25 workgroups
    hipLaunchKernelGGL(resae_bwd_data_final_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st, (const float*)ws, add, dx, N,
                       Cin, H, W, kind == K3UP ? 1 : 0, ncib * 16, q.splits);
    rc = check_launch("resae_bwd_data (final)");
  }
  return rc;
}

size_t wfae_resae_bwd_weight_workspace_bytes(int route, int kind, int N, int Cin, int Cout, int H, int W) {
  if (check_layer("resae_bwd_weight_workspace_bytes", route, kind, N, Cin, Cout, H, W)) return 0;
  return plan_weight(route, kind, N, Cin, Cout, H, W).ws;
}

int wfae_resae_bwd_weight(const float* dy, const float* x, float* dw, float* dbias, int route, int kind, int N, int Cin, int Cout,
                          int H, int W, void* ws, size_t ws_bytes, wfae_stream_t stream) {
  WFAE_REQUIRE(dy && x && dw, WFAE_ERR_NULL_POINTER, "resae_bwd_weight: null pointer");
  int rc = check_layer("resae_bwd_weight", route, kind, N, Cin, Cout, H, W);
  if (rc) return rc;
  const Plan q = plan_weight(route, kind, N, Cin, Cout, H, W);
  if ((rc = check_ws("resae_bwd_weight", q, ws, ws_bytes))) return rc;
  WFAE_REQUIRE(q.splits <= 65535, WFAE_ERR_BAD_SHAPE, "resae_bwd_weight: grid too large");
  WP p = {};
  p.dy = dy; p.x = x; p.out = q.splits > 1 ? (float*)ws : dw; p.g = q.g;
  p.Cin = Cin; p.Cout = Cout; p.Ho = out_size(kind, H); p.Wo = out_size(kind, W); p.T = kind_taps(kind);
  p.per_split = q.per_split; p.live = live_mask(kind, H, W);
  p.slab = (long)Cout * Cin * p.T;
  hipStream_t st = (hipStream_t)stream;
  (void)hipFuncSetAttribute((const void*)resae_bwd_weight_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)kLdsLimit);
  hipLaunchKernelGGL(resae_bwd_weight_kernel, dim3(cdiv(Cin, CK), cdiv(Cout, 64), q.splits), dim3(kThreads), q.lds, st, p);
  if ((rc = check_launch("resae_bwd_weight"))) return rc;
  if (q.splits > 1) {
    hipLaunchKernelGGL(resae_bwd_weight_final_kernel, dim3((unsigned)((p.slab + 255) / 256)), dim3(256), 0, st, (const float*)ws, dw, p.slab,
                       q.splits);
    if ((rc = check_launch("resae_bwd_weight (final)"))) return rc;
  }
  if (dbias) {
    hipLaunchKernelGGL(resae_bwd_bias_kernel, dim3(Cout), dim3(256), 0, st, dy, dbias, N, Cout, (long)p.Ho * p.Wo);
    rc = check_launch("resae_bwd_weight (bias)");
  }
  return rc;
}

int wfae_resae_join_fwd(const float* c2, const float* s2, const float* h2, const float* r, const float* ss, const float* hs, float* y,
                        int res_mode, int N, int C, int H, int W, wfae_stream_t stream) {
  WFAE_REQUIRE(c2 && s2 && h2 && r && y, WFAE_ERR_NULL_POINTER, "resae_join_fwd: null pointer");
  int rc = check_join("resae_join_fwd", res_mode, N, C, H, W, (ss != nullptr) == (hs != nullptr));
  if (rc) return rc;
  JP p = {};
  p.c2 = c2; p.s2 = s2; p.h2 = h2; p.r = r; p.ss = ss; p.hs = hs; p.y = y; p.C = C; p.H = H; p.W = W; p.res_mode = res_mode;
  return launch_join<false>(p, N, (hipStream_t)stream, "resae_join_fwd");
}

int wfae_resae_join_bwd(const float* dy, const float* c2, const float* s2, const float* h2, const float* r, const float* ss,
                        const float* hs, float* dpre, float* dres, int res_mode, int N, int C, int H, int W, wfae_stream_t stream) {
  WFAE_REQUIRE(dy && c2 && s2 && h2 && r && dpre, WFAE_ERR_NULL_POINTER, "resae_join_bwd: null pointer");
  int rc = check_join("resae_join_bwd", res_mode, N, C, H, W, (ss != nullptr) == (hs != nullptr));
  if (rc) return rc;
  WFAE_REQUIRE((dres != nullptr) == (res_mode == 2), WFAE_ERR_BAD_SHAPE,
               "resae_join_bwd: dres goes with res_mode 2 exactly (at res_mode 1 the residual's gradient is dpre)");
  JP p = {};
  p.dy = dy; p.c2 = c2; p.s2 = s2; p.h2 = h2; p.r = r; p.ss = ss; p.hs = hs; p.dpre = dpre; p.dres = dres;
  p.C = C; p.H = H; p.W = W; p.res_mode = res_mode;
  return launch_join<true>(p, N, (hipStream_t)stream, "resae_join_bwd");
}

int wfae_resae_bn_running(const float* save_mean, const float* save_invstd, float* running_mean, float* running_var, int C, float eps,
                          float momentum, int64_t count, wfae_stream_t stream) {
  WFAE_REQUIRE(save_mean && save_invstd && running_mean && running_var, WFAE_ERR_NULL_POINTER, "resae_bn_running: null pointer");
  WFAE_REQUIRE(C > 0 && count > 0 && eps > 0.f, WFAE_ERR_BAD_SHAPE, "resae_bn_running: bad arguments C=%d count=%lld", C, (long long)count);
  hipLaunchKernelGGL(resae_bn_running_kernel, dim3(cdiv(C, 128)), dim3(128), 0, (hipStream_t)stream, save_mean, save_invstd, running_mean,
                     running_var, C, eps, momentum, (double)count);
  return check_launch("resae_bn_running");
}

}  // extern "C"
