// prediff.hip — kernels of the intensity-statistics MLP forecaster (reference experiments/v1_experiments/
// prediff_mlp_sevir/train.py:20-38 `MLP`, :56-70 training_step): the per-frame means and per-group mean / standard
// deviation of a raw (B, 25, H, W) sequence batch in one read of the batch, and the whole
// Linear-ReLU-Linear-ReLU-Linear + MSE step (forward, loss, all six parameter gradients) in one launch.
//
// Statistics.  Nothing is ever formed as E[x^2] - E[x]^2.  A workgroup owns a piece of one sample, keeps it in
// registers, and leaves (count, mean, M2) partials; a second launch pools them in fp64 (the K-way form of Chan's
// update, pool_by_frame below) in a fixed order: partials -> frames -> groups.  Two memory orders:
//   frames contiguous (B, T, HW): a piece is the part of one frame inside one 8192-float window of the buffer (windows
//     are anchored at a 16-byte aligned address, so every load of a whole quad is an aligned 16-byte load whatever the
//     frame's own alignment; the edge quads of a piece are read element by element).  Two passes over the registers:
//     block sum -> mean, then the squares about the mean rounded to fp32 (the rounding is taken out again exactly).
//   T innermost (B, HW, T): reads stay contiguous (1 KiB per wave instruction) and the frame of an element is its
//     index % T.  A workgroup takes every T-th 1024-float row of a tile of kRows * T rows, so the four elements a
//     lane loads belong to the same four frames in every row: four register streams per lane, each summed shifted by
//     its first element (the shift is one of the stream's own values, so the cancellation in S2 - S1^2 / n is bounded
//     by the stream length), then pooled by frame through LDS in a fixed order.
// No atomics anywhere: repeated calls give identical bits.
#include "common.h"

using namespace wfae;

namespace {

constexpr int kST = 256;                    // threads of a statistics workgroup
constexpr int kQuads = 8;                   // 16-byte loads per thread, frames-contiguous order
constexpr int kChunk = kST * kQuads * 4;    // 8192 floats: the window a workgroup reduces in that order
constexpr int kRow = kST * 4;               // 1024 floats: one workgroup-wide load
constexpr int kRows = 16;                   // rows per workgroup, T-innermost order
constexpr int kMaxT = 256;

// The pooled moments of K pieces (n_k, mean_k, M2_k) — the K-way form of Chan, Golub and LeVeque's update:
//   n = sum n_k,  mean = sum n_k mean_k / n,  M2 = sum (M2_k + n_k (mean_k - mean)^2)
// Two sums in fp64 and one division; nothing depends on the piece before it.  For every frame t < T at once, by a
// workgroup of kST threads: P = kST / T threads share a frame (piece k goes to thread k % P, ascending k) and the first
// of them adds their partial sums in ascending order.  load(t, k, n, mean, m2) fetches a piece (n = 0: empty),
// done(t, n, mean, m2) receives the result in one thread per frame.  sm: 2 kST + T doubles of LDS.
template <class Load, class Done>
__device__ __forceinline__ void pool_by_frame(int T, int K, double* sm, Load load, Done done) {
  const int P = kST / T;
  const int t = threadIdx.x / P, part = threadIdx.x % P;
  const bool act = t < T;
  double* sa = sm;
  double* sb = sm + kST;
  double* smean = sm + 2 * kST;
  double cnt = 0.0, sum = 0.0;
  if (act)
    for (int k = part; k < K; k += P) {
      double n, m, m2;
      load(t, k, n, m, m2);
      cnt += n;
      sum += n * m;
    }
  sa[threadIdx.x] = cnt;
  sb[threadIdx.x] = sum;
  __syncthreads();
  double ntot = 0.0, mean = 0.0;
  if (act && part == 0) {
    double s = 0.0;
    for (int j = 0; j < P; ++j) {
      ntot += sa[threadIdx.x + j];
      s += sb[threadIdx.x + j];
    }
    mean = ntot > 0.0 ? s / ntot : 0.0;
    smean[t] = mean;
  }
  __syncthreads();
  double q = 0.0;
  if (act) {
    const double mt = smean[t];
    for (int k = part; k < K; k += P) {
      double n, m, m2;
      load(t, k, n, m, m2);
      const double d = m - mt;
      q += m2 + n * d * d;
    }
  }
  sa[threadIdx.x] = q;
  __syncthreads();
  if (act && part == 0) {
    double m2 = 0.0;
    for (int j = 0; j < P; ++j) m2 += sa[threadIdx.x + j];
    done(t, ntot, mean, m2);
  }
}

// frames contiguous.  Workgroup (f, j): frame f = b * T + t occupies floats [mis + f HW, mis + (f + 1) HW) of `base`
// (16-byte aligned; mis = the tensor's offset from it in floats); its j-th window is [w0, w0 + kChunk),
// w0 = (start / kChunk + j) * kChunk.  part[3 (f K0 + j)] = (count, mean, M2) of the frame's elements in the window.
__global__ __launch_bounds__(kST) void stats_frames_kernel(const float* __restrict__ base, int mis, long HW, int K0,
                                                           double* __restrict__ part) {
  __shared__ double red[16];
  __shared__ double bc;
  const long f = blockIdx.x / K0;
  const int j = blockIdx.x % K0;
  const long fs = mis + f * HW, fe = fs + HW;
  const long w0 = (fs / kChunk + j) * (long)kChunk;
  const long lo = fs > w0 ? fs : w0, hi = fe < w0 + kChunk ? fe : w0 + kChunk;
  double* out = part + 3 * (long)blockIdx.x;
  if (lo >= hi) {   // the frame ends before this window (uniform for the workgroup)
    if (threadIdx.x == 0) out[0] = out[1] = out[2] = 0.0;
    return;
  }
  float v[kQuads][4];
  unsigned valid = 0;
#pragma unroll
  for (int q = 0; q < kQuads; ++q) {
    const long p = w0 + (long)(q * kST + threadIdx.x) * 4;
    if (p >= lo && p + 4 <= hi) {
      ldv(base + p, v[q]);
      valid |= 0xFu << (4 * q);
    } else {
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const bool in = p + e >= lo && p + e < hi;
        v[q][e] = in ? base[p + e] : 0.f;
        valid |= (in ? 1u : 0u) << (4 * q + e);
      }
    }
  }
  double s = 0.0;
#pragma unroll
  for (int q = 0; q < kQuads; ++q) s += (double)((v[q][0] + v[q][1]) + (v[q][2] + v[q][3]));
  const double n = (double)(hi - lo);
  const double tot = block_sum(s, red);
  if (threadIdx.x == 0) bc = tot / n;
  __syncthreads();
  const double mean = bc;
  const float mf = (float)mean;
  double s2 = 0.0;
#pragma unroll
  for (int q = 0; q < kQuads; ++q) {
    float q4 = 0.f;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const float d = (valid >> (4 * q + e)) & 1u ? v[q][e] - mf : 0.f;
      q4 = fmaf(d, d, q4);
    }
    s2 += (double)q4;
  }
  const double m2f = block_sum(s2, red);   // sum of squares about mf = M2 + n (mean - mf)^2
  if (threadIdx.x == 0) {
    const double dm = mean - (double)mf;
    const double m2 = m2f - n * dm * dm;
    out[0] = n;
    out[1] = mean;
    out[2] = m2 > 0.0 ? m2 : 0.0;
  }
}

// T innermost.  Sample b occupies floats [sb, sb + N) of `base`, sb = mis + b N, N = HW T; rows of kRow floats are
// counted from ab = sb rounded down to a multiple of 4.  Workgroup (b, tile, r), r < T, reads rows (tile kRows + it) T + r,
// it < kRows.  part[3 ((b KB + tile T + r) T + t)] = (count, mean, M2) of frame t's elements among them, KB = tiles T.
__global__ __launch_bounds__(kST) void stats_tinner_kernel(const float* __restrict__ base, int mis, long N, int T,
                                                           int tiles, double* __restrict__ part) {
  __shared__ double s_mean[kRow];
  __shared__ float s_m2[kRow];
  __shared__ float s_cnt[kRow];
  __shared__ double s_pool[2 * kST + kMaxT];
  const int r = blockIdx.x % T;
  const long bt = blockIdx.x / T;
  const int tile = (int)(bt % tiles);
  const long b = bt / tiles;
  const long sb = mis + b * N, se = sb + N;
  const long ab = sb & ~3L;
  const long row0 = ab + ((long)tile * kRows * T + r) * kRow;   // first float of the workgroup's first row
  const long step = (long)T * kRow;
  float v0[4], s1[4] = {0.f, 0.f, 0.f, 0.f}, s2[4] = {0.f, 0.f, 0.f, 0.f};
  int cnt[4] = {0, 0, 0, 0};
  float v[kRows][4];
  unsigned valid[4] = {0, 0, 0, 0};   // bit `it` of valid[e]: element e of row `it` belongs to the sample
#pragma unroll
  for (int it = 0; it < kRows; ++it) {
    const long p = row0 + it * step + threadIdx.x * 4;
    if (p >= sb && p + 4 <= se) {
      ldv(base + p, v[it]);
#pragma unroll
      for (int e = 0; e < 4; ++e) valid[e] |= 1u << it;
    } else {
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const bool in = p + e >= sb && p + e < se;
        v[it][e] = in ? base[p + e] : 0.f;
        valid[e] |= (in ? 1u : 0u) << it;
      }
    }
  }
  // all rows inside the sample (uniform; true for all but the first and last workgroups of a sample): no masks
  const bool full = row0 >= sb && row0 + (kRows - 1) * step + kRow <= se;
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    if (full) {
      v0[e] = v[0][e];
#pragma unroll
      for (int it = 1; it < kRows; ++it) {
        const float d = v[it][e] - v0[e];
        s1[e] += d;
        s2[e] = fmaf(d, d, s2[e]);
      }
      cnt[e] = kRows;
    } else {
      v0[e] = 0.f;
      bool have = false;
#pragma unroll
      for (int it = 0; it < kRows; ++it) {
        const bool in = (valid[e] >> it) & 1u;
        if (in && !have) {
          v0[e] = v[it][e];
          have = true;
        }
      }
#pragma unroll
      for (int it = 0; it < kRows; ++it) {
        const bool in = (valid[e] >> it) & 1u;
        const float d = in ? v[it][e] - v0[e] : 0.f;
        s1[e] += d;
        s2[e] = fmaf(d, d, s2[e]);
        cnt[e] += in ? 1 : 0;
      }
    }
    const int i = threadIdx.x * 4 + e;
    // 1 / count (count <= kRows) to fp64 accuracy: one Newton step on the fp32 reciprocal, no fp64 division
    const double c = (double)cnt[e];
    double inv = (double)__builtin_amdgcn_rcpf((float)(cnt[e] ? cnt[e] : 1));
    inv = inv * (2.0 - c * inv);
    const double m = cnt[e] ? (double)v0[e] + (double)s1[e] * inv : 0.0;
    const double m2 = cnt[e] ? (double)s2[e] - (double)s1[e] * (double)s1[e] * inv : 0.0;
    s_cnt[i] = (float)cnt[e];
    s_mean[i] = m;
    s_m2[i] = m2 > 0.0 ? (float)m2 : 0.f;
  }
  __syncthreads();
  // LDS index i holds the elements at floats row0 + i (+ multiples of T kRow): frame (row0 + i - sb) mod T
  long c0 = (row0 - sb) % T;
  if (c0 < 0) c0 += T;
  double* out = part + 3 * (long)blockIdx.x * T;
  pool_by_frame(
      T, (kRow + T - 1) / T, s_pool,
      [&](int t, int k, double& n, double& m, double& m2) {
        int i0 = (t - (int)c0) % T;
        if (i0 < 0) i0 += T;
        const int i = i0 + k * T;
        const bool in = i < kRow;
        n = in ? (double)s_cnt[i] : 0.0;
        m = in ? s_mean[i] : 0.0;
        m2 = in ? (double)s_m2[i] : 0.0;
      },
      [&](int t, double n, double m, double m2) {
        out[3 * t] = n;
        out[3 * t + 1] = m;
        out[3 * t + 2] = m2;
      });
}

// partial (b, t, k) sits at part[3 (b sb + t st + k sk)], k < K.  Workgroup (b, j) of kST threads: j < groups pools
// the pieces of each frame of group j, then those frames, into the group's mean and std; j = groups pools each of the
// t_in input frames into x.  Pieces and frames are taken in ascending order.
__global__ __launch_bounds__(kST) void stats_merge_kernel(const double* __restrict__ part, long sb, long st, long sk,
                                                          int K, int T, int t_in, int groups, float* __restrict__ x,
                                                          float* __restrict__ target) {
  __shared__ double s_pool[2 * kST + kMaxT];
  __shared__ double fr[3 * kMaxT];   // (n, mean, m2) per frame of this workgroup
  const long b = blockIdx.x / (groups + 1);
  const int j = blockIdx.x % (groups + 1);
  const int per = (T - t_in) / groups;
  const int t0 = j < groups ? t_in + j * per : 0, tn = j < groups ? per : t_in;
  pool_by_frame(
      tn, K, s_pool,
      [&](int t, int k, double& n, double& m, double& m2) {
        const double* p = part + 3 * (b * sb + (long)(t0 + t) * st + (long)k * sk);
        n = p[0];
        m = p[1];
        m2 = p[2];
      },
      [&](int t, double n, double m, double m2) {
        fr[3 * t] = n;
        fr[3 * t + 1] = m;
        fr[3 * t + 2] = m2;
        if (j == groups) x[b * t_in + t] = (float)m;
      });
  __syncthreads();
  if (j < groups && threadIdx.x == 0) {
    double n = 0.0, sum = 0.0, m2 = 0.0;
    for (int t = 0; t < per; ++t) {
      n += fr[3 * t];
      sum += fr[3 * t] * fr[3 * t + 1];
    }
    const double mean = sum / n;
    for (int t = 0; t < per; ++t) {
      const double d = fr[3 * t + 1] - mean;
      m2 += fr[3 * t + 2] + fr[3 * t] * d * d;
    }
    target[b * 2 * groups + j] = (float)mean;
    target[b * 2 * groups + groups + j] = (float)sqrt(m2 / (n - 1.0));   // n = 1: nan, as torch.std
  }
}

// ---- Linear-ReLU-Linear-ReLU-Linear + MSE in one workgroup ----------------------------------------------------------
constexpr int kMT = 1024;   // threads of the MLP workgroup
constexpr int kKT = 32;     // reduction chunk of the LDS tiles
constexpr int kBT = 16;     // batch chunk of the weight gradients
constexpr int kMaxH = 256, kMaxB = 64;
constexpr int kNW = kMaxH * kKT / kMT;    // weight-tile elements a thread carries from global memory to LDS
constexpr int kNX = kMaxB * kKT / kMT;    // the same for the activation tile
constexpr int kSW = kMaxH * (kKT + 1);    // floats of the weight tile (rows up to 257 apart), >= kBT * 2 kMaxH
constexpr int kSX = kMaxB * kKT;

struct MlpArgs {
  const float *x, *tgt, *w1, *b1, *w2, *b2, *w3, *b3;
  float *pred, *loss, *dw1, *db1, *dw2, *db2, *dw3, *db3;
  float* ws;
  int B, I, H, O, fwd_only;
};

// ep(b, j, sum_r W(j, r) in[b * ldin + r]) for b < B, j < J, r < R; a thread owns output j for CB batch rows.
// OUT_ROWS: W(j, r) = W[j * ld + r] (forward: a row of W is an output) else W[r * ld + j] (data gradient: a row is a
// reduction index).  Nothing in the inner loop touches global memory: KT reduction indices at a time, W goes to the LDS
// tile sw[rr][j] (loaded along the contiguous axis of W; odd row stride, so both the transposing store of the forward
// and the reads along j are conflict-free) and `in` to sx[b][rr] (read as broadcasts; rows b >= B hold zeros); the next
// tile is already on its way to registers while the current one is multiplied.  `in` may have been written by other
// threads of this workgroup before the last barrier (no __restrict__).
template <int CB, bool OUT_ROWS, class Ep>
__device__ __forceinline__ void dense(const float* __restrict__ W, int ld, const float* in, int ldin, int B, int J, int R,
                                      float* sw, float* sx, Ep ep) {
  const int JS = J | 1;
  const int nbc = (B + CB - 1) / CB;
  const int items = J * nbc;
  // tile depth KT: the largest power of two (>= kKT) of reduction indices that both tiles hold, so a narrow map takes
  // fewer trips.  One workgroup on one CU is bound by instruction issue: every index below is formed once per call
  // (shifts for the power of two, one division by J carried forward by increments), not once per tile.
  const int cap_r = kNW * kMT / J, cap_l = kSW / JS, cap_x = kSX / (nbc * CB);
  const int cap = cap_r < cap_l ? (cap_r < cap_x ? cap_r : cap_x) : (cap_l < cap_x ? cap_l : cap_x);
  const int lg = 31 - __builtin_clz(cap), KT = 1 << lg;
  constexpr int kOut = 1 << 30;   // "not part of the tile"
  int goff[kNW], loff[kNW], wrr[kNW], xoff[kNX], xrr[kNX];
  {
    int jj = OUT_ROWS ? 0 : threadIdx.x % J, rr = OUT_ROWS ? 0 : threadIdx.x / J;
    const int dj = kMT % J, dr = kMT / J;
#pragma unroll
    for (int u = 0; u < kNW; ++u) {
      const int i = threadIdx.x + u * kMT;
      if (OUT_ROWS) {
        rr = i & (KT - 1);
        jj = i >> lg;
      }
      const bool ok = OUT_ROWS ? jj < J : rr < KT;
      goff[u] = OUT_ROWS ? jj * ld + rr : rr * ld + jj;
      loff[u] = rr * JS + jj;
      wrr[u] = ok ? rr : kOut;
      if (!OUT_ROWS) {
        jj += dj;
        rr += dr;
        if (jj >= J) {
          jj -= J;
          ++rr;
        }
      }
    }
#pragma unroll
    for (int u = 0; u < kNX; ++u) {
      const int i = threadIdx.x + u * kMT;
      const int rr = i & (KT - 1), bb = i >> lg;
      xoff[u] = bb * ldin + rr;
      xrr[u] = bb < B ? rr : kOut;
    }
  }
  float pw[kNW], px[kNX];
  auto fetch = [&](int r0) {
    const float* __restrict__ wt = W + (OUT_ROWS ? r0 : r0 * ld);
#pragma unroll
    for (int u = 0; u < kNW; ++u) pw[u] = wrr[u] < R - r0 ? wt[goff[u]] : 0.f;
#pragma unroll
    for (int u = 0; u < kNX; ++u) px[u] = xrr[u] < R - r0 ? in[r0 + xoff[u]] : 0.f;
  };
  for (int base = 0; base < items; base += kMT) {
    const int item = base + threadIdx.x;
    const bool act = item < items;
    const int j = act ? item % J : 0, b0 = act ? (item / J) * CB : 0;
    float acc[CB];
#pragma unroll
    for (int c = 0; c < CB; ++c) acc[c] = 0.f;
    fetch(0);
    for (int r0 = 0; r0 < R; r0 += KT) {
      __syncthreads();   // the tile of the step before has been read
#pragma unroll
      for (int u = 0; u < kNW; ++u)
        if (wrr[u] != kOut) sw[loff[u]] = pw[u];
#pragma unroll
      for (int u = 0; u < kNX; ++u) sx[threadIdx.x + u * kMT] = px[u];
      __syncthreads();
      if (r0 + KT < R) fetch(r0 + KT);
      const int rn = R - r0 < KT ? R - r0 : KT;
      const float* swj = sw + j;
      const float* sxb = sx + b0 * KT;
#pragma unroll 2
      for (int rr = 0; rr < rn; ++rr) {
        const float wv = swj[rr * JS];
#pragma unroll
        for (int c = 0; c < CB; ++c) acc[c] = fmaf(wv, sxb[c * KT + rr], acc[c]);
      }
    }
#pragma unroll
    for (int c = 0; c < CB; ++c)
      if (act && b0 + c < B) ep(b0 + c, j, acc[c]);
  }
}

// dW[o][k] = sum_b d[b][o] in[b][k], db[o] = sum_b d[b][o], b ascending.  kBT batch rows of d and `in` at a time are
// staged in LDS; a thread keeps the same elements of dW in every chunk, so the later chunks add to what it wrote.
__device__ __forceinline__ void dense_bwd_weight(const float* d, const float* in, float* __restrict__ dW,
                                                 float* __restrict__ db, int B, int K, int O, float* sw) {
  float* sd = sw;
  float* si = sw + kBT * O;
  for (int b0 = 0; b0 < B; b0 += kBT) {
    const int bn = B - b0 < kBT ? B - b0 : kBT;
    __syncthreads();
    for (int i = threadIdx.x; i < bn * O; i += kMT) sd[i] = d[b0 * O + i];
    for (int i = threadIdx.x; i < bn * K; i += kMT) si[i] = in[b0 * K + i];
    __syncthreads();
    int o = threadIdx.x / K, k = threadIdx.x % K;   // (o, k) of the thread's item, carried forward by increments
    const int dk = kMT % K, dO = kMT / K;
    for (int item = threadIdx.x; item < O * K; item += kMT) {
      float acc = 0.f;
      for (int bb = 0; bb < bn; ++bb) acc = fmaf(sd[bb * O + o], si[bb * K + k], acc);
      dW[item] = b0 == 0 ? acc : dW[item] + acc;
      k += dk;
      o += dO;
      if (k >= K) {
        k -= K;
        ++o;
      }
    }
    for (int o = threadIdx.x; o < O; o += kMT) {
      float acc = 0.f;
      for (int bb = 0; bb < bn; ++bb) acc += sd[bb * O + o];
      db[o] = b0 == 0 ? acc : db[o] + acc;
    }
  }
}

// CB: batch rows per thread in the forward / data-gradient maps: 1 keeps all 1024 threads busy at small B, 2 fits the
// registers of a 1024-thread workgroup without spilling
template <int CB>
__global__ __launch_bounds__(kMT) void mlp3_mse_kernel(MlpArgs a) {
  __shared__ double red[16];
  __shared__ float sw[kSW];
  __shared__ float sx[kSX];
  const int B = a.B, I = a.I, H = a.H, O = a.O;
  float* h1 = a.ws;               // (B, H) relu(W1 x + b1)
  float* h2 = h1 + B * H;         // (B, H) relu(W2 h1 + b2)
  float* dz2 = h2 + B * H;        // (B, H)
  float* dz1 = dz2 + B * H;       // (B, H)
  float* d3 = dz1 + B * H;        // (B, O) d loss / d pred
  dense<CB, true>(a.w1, I, a.x, I, B, H, I, sw, sx,
                  [&](int b, int j, float v) { h1[b * H + j] = fmaxf(v + a.b1[j], 0.f); });
  __syncthreads();
  dense<CB, true>(a.w2, H, h1, H, B, H, H, sw, sx,
                  [&](int b, int j, float v) { h2[b * H + j] = fmaxf(v + a.b2[j], 0.f); });
  __syncthreads();
  dense<CB, true>(a.w3, H, h2, H, B, O, H, sw, sx, [&](int b, int j, float v) { a.pred[b * O + j] = v + a.b3[j]; });
  if (!a.tgt) return;
  __syncthreads();
  const int n = B * O;
  const float gscale = 2.f / (float)n;
  double s = 0.0;
  for (int i = threadIdx.x; i < n; i += kMT) {
    const float d = a.pred[i] - a.tgt[i];
    s += (double)d * d;
    if (!a.fwd_only) d3[i] = gscale * d;
  }
  const double tot = block_sum(s, red);
  if (threadIdx.x == 0) a.loss[0] = (float)(tot / (double)n);
  if (a.fwd_only) return;
  __syncthreads();
  dense<CB, false>(a.w3, H, d3, O, B, H, O, sw, sx,
                   [&](int b, int j, float v) { dz2[b * H + j] = h2[b * H + j] > 0.f ? v : 0.f; });
  __syncthreads();
  dense<CB, false>(a.w2, H, dz2, H, B, H, H, sw, sx,
                   [&](int b, int j, float v) { dz1[b * H + j] = h1[b * H + j] > 0.f ? v : 0.f; });
  dense_bwd_weight(d3, h2, a.dw3, a.db3, B, H, O, sw);
  dense_bwd_weight(dz2, h1, a.dw2, a.db2, B, H, H, sw);
  dense_bwd_weight(dz1, a.x, a.dw1, a.db1, B, I, H, sw);
}

int stats_plan(const char* what, int B, int T, int64_t HW, int t_innermost, long* k_per_frame, long* blocks) {
  WFAE_REQUIRE(B > 0 && T > 0 && HW > 0, WFAE_ERR_BAD_SHAPE, "%s: bad shape B=%d T=%d HW=%lld", what, B, T,
               (long long)HW);
  WFAE_REQUIRE(T <= kMaxT, WFAE_ERR_UNSUPPORTED, "%s: T=%d frames, at most %d are served", what, T, kMaxT);
  WFAE_REQUIRE(HW <= ((int64_t)1 << 40) / T, WFAE_ERR_BAD_SHAPE, "%s: HW=%lld too large", what, (long long)HW);
  long k, nb;
  if (t_innermost) {
    const int64_t span = (int64_t)kRows * T * kRow;
    const int64_t tiles = (HW * T + 3 + span - 1) / span;
    k = (long)(tiles * T);               // partials per (sample, frame)
    nb = (long)B * k;
  } else {
    k = (long)((HW + kChunk - 1) / kChunk + 1);   // windows a frame can touch
    nb = (long)B * T * k;
  }
  WFAE_REQUIRE(nb < ((long)1 << 31), WFAE_ERR_BAD_SHAPE, "%s: B=%d T=%d HW=%lld needs %ld workgroups", what, B, T,
               (long long)HW, nb);
  *k_per_frame = k;
  *blocks = nb;
  return 0;
}

}  // namespace

extern "C" {

size_t wfae_seq_intensity_stats_ws_bytes(int B, int T, int64_t HW, int t_innermost) {
  long k, nb;
  if (stats_plan("seq_intensity_stats_ws_bytes", B, T, HW, t_innermost, &k, &nb)) return 0;
  return (size_t)B * T * k * 3 * sizeof(double);
}

int wfae_seq_intensity_stats(const float* seq, float* x, float* target, int B, int T, int64_t HW, int t_in, int groups,
                             int t_innermost, void* ws, size_t ws_bytes, wfae_stream_t stream) {
  WFAE_REQUIRE(seq && x && target, WFAE_ERR_NULL_POINTER, "seq_intensity_stats: null pointer");
  long k, nb;
  int rc = stats_plan("seq_intensity_stats", B, T, HW, t_innermost, &k, &nb);
  if (rc) return rc;
  WFAE_REQUIRE(t_in > 0 && t_in < T && groups > 0, WFAE_ERR_BAD_SHAPE,
               "seq_intensity_stats: bad split T=%d t_in=%d groups=%d", T, t_in, groups);
  WFAE_REQUIRE((T - t_in) % groups == 0, WFAE_ERR_BAD_SHAPE,
               "seq_intensity_stats: pred_frames = %d is not a multiple of groups = %d (a group is a chunk of "
               "pred_frames * H * W / groups consecutive elements; only whole frames are served)", T - t_in, groups);
  WFAE_REQUIRE((reinterpret_cast<uintptr_t>(seq) & 3) == 0, WFAE_ERR_BAD_SHAPE,
               "seq_intensity_stats: seq must be 4-byte aligned");
  const size_t need = (size_t)B * T * k * 3 * sizeof(double);
  WFAE_REQUIRE(ws && ws_bytes >= need, WFAE_ERR_WORKSPACE, "seq_intensity_stats: workspace too small (%zu < %zu)",
               ws_bytes, need);
  WFAE_REQUIRE((reinterpret_cast<uintptr_t>(ws) & 7) == 0, WFAE_ERR_WORKSPACE,
               "seq_intensity_stats: workspace must be 8-byte aligned");
  hipStream_t st = (hipStream_t)stream;
  const uintptr_t addr = reinterpret_cast<uintptr_t>(seq);
  const float* base = reinterpret_cast<const float*>(addr & ~(uintptr_t)15);
  const int mis = (int)((addr & 15) >> 2);
  double* part = (double*)ws;
  if (t_innermost) {
    // the plan allows a sample to start 3 floats past a 16-byte boundary; this call knows where its samples start
    const int64_t N = HW * T, span = (int64_t)kRows * T * kRow;
    const int tiles = (int)((N + (N % 4 ? 3 : mis) + span - 1) / span);
    k = (long)tiles * T;
    hipLaunchKernelGGL(stats_tinner_kernel, dim3((unsigned)(B * k)), dim3(kST), 0, st, base, mis, (long)N, T, tiles,
                       part);
    if ((rc = check_launch("seq_intensity_stats_part"))) return rc;
    hipLaunchKernelGGL(stats_merge_kernel, dim3(B * (groups + 1)), dim3(kST), 0, st, (const double*)part,
                       k * T, 1L, (long)T, (int)k, T, t_in, groups, x, target);
  } else {
    hipLaunchKernelGGL(stats_frames_kernel, dim3((unsigned)nb), dim3(kST), 0, st, base, mis, (long)HW, (int)k, part);
    if ((rc = check_launch("seq_intensity_stats_part"))) return rc;
    hipLaunchKernelGGL(stats_merge_kernel, dim3(B * (groups + 1)), dim3(kST), 0, st, (const double*)part,
                       (long)T * k, k, 1L, (int)k, T, t_in, groups, x, target);
  }
  return check_launch("seq_intensity_stats");
}

int wfae_mlp3_mse(const float* x, const float* target, const float* w1, const float* b1, const float* w2,
                  const float* b2, const float* w3, const float* b3, float* pred, float* loss, float* dw1, float* db1,
                  float* dw2, float* db2, float* dw3, float* db3, int B, int in, int hidden, int out, int forward_only,
                  void* ws, size_t ws_bytes, wfae_stream_t stream) {
  WFAE_REQUIRE(x && w1 && b1 && w2 && b2 && w3 && b3 && pred, WFAE_ERR_NULL_POINTER, "mlp3_mse: null pointer");
  if (forward_only)
    WFAE_REQUIRE((target == nullptr) == (loss == nullptr), WFAE_ERR_NULL_POINTER,
                 "mlp3_mse: forward_only takes target and loss together or neither");
  else
    WFAE_REQUIRE(target && loss && dw1 && db1 && dw2 && db2 && dw3 && db3, WFAE_ERR_NULL_POINTER,
                 "mlp3_mse: null pointer (target, loss and the six gradients are needed unless forward_only)");
  WFAE_REQUIRE(B > 0 && in > 0 && hidden > 0 && out > 0, WFAE_ERR_BAD_SHAPE,
               "mlp3_mse: bad shape B=%d in=%d hidden=%d out=%d", B, in, hidden, out);
  WFAE_REQUIRE(in <= 32 && out <= 32 && hidden <= kMaxH && B <= kMaxB, WFAE_ERR_UNSUPPORTED,
               "mlp3_mse: B=%d in=%d hidden=%d out=%d: one workgroup carries the whole step, served up to B = 64, "
               "in = 32, hidden = 256, out = 32", B, in, hidden, out);
  const size_t need = (forward_only ? (size_t)2 * B * hidden : (size_t)4 * B * hidden + (size_t)B * out) * sizeof(float);
  WFAE_REQUIRE(ws && ws_bytes >= need, WFAE_ERR_WORKSPACE, "mlp3_mse: workspace too small (%zu < %zu)", ws_bytes, need);
  MlpArgs a{x, target, w1, b1, w2, b2, w3, b3, pred, loss, dw1, db1, dw2, db2, dw3, db3, (float*)ws,
            B, in, hidden, out, forward_only ? 1 : 0};
  if (B * hidden <= 2 * kMT)
    hipLaunchKernelGGL(mlp3_mse_kernel<1>, dim3(1), dim3(kMT), 0, (hipStream_t)stream, a);
  else
    hipLaunchKernelGGL(mlp3_mse_kernel<2>, dim3(1), dim3(kMT), 0, (hipStream_t)stream, a);
  return check_launch("mlp3_mse");
}

}  // extern "C"
