// skill.hip — forecast-skill scores of the reference's pipeline/metrics.py (:9-68): the contingency counts behind
// CSI / HSS (`_hit_miss_fa_cn` at up to 8 thresholds) and the CRPS sum of a Gaussian ensemble, for up to 3 poolings
// (none / avg / max, F.*_pool2d(s, stride=s)), in one pass over pred and target.
//
// Counts are compared bit for bit with the reference, so every pooled value is formed in exactly the order torch forms
// it on the CPU: an s x s average is the row-major sequential fp32 sum of the window followed by a true division by
// s^2; an ensemble mean is the sequential fp32 sum over the members followed by a true division by N.  No tree sums,
// no reciprocal multiplies (hipcc's default fp32 division is correctly rounded; -ffp-contract=on leaves plain adds
// alone).  Each lane owns one pooled cell; blocks write partial rows and a finalize kernel reduces them in a fixed
// order — no atomics, so results are bitwise repeatable.
#include "common.h"

using namespace wfae;

namespace {

constexpr int kBlock = 256;
constexpr int kMaxPools = 3, kMaxThr = 8;
constexpr int kRow = 3 * kMaxThr + 1;   // partial row of a block: tp/fn/fp per threshold (uint64), CRPS sum (double
                                        // bits); the rows are stored column-major in the workspace
constexpr int kMaxBlocksPerPool = 1024;
constexpr int kFinal = 256;    // finalize block (1024 threads measured slower: 18 us against 12.7 us)

struct SkillCfg {
  int n_pools, n_thr;
  int type[kMaxPools];    // 0 none, 1 avg, 2 max
  int scale[kMaxPools];
  int blk_lo[kMaxPools], blk_hi[kMaxPools];   // block range of each pool in the grid
  float thr[kMaxThr];
};

__device__ __forceinline__ float clamp01f(float v) { return fminf(fmaxf(v, 0.f), 1.f); }

// pooled value of one s x s window of one plane, row-major sequential (avg: then / s^2)
__device__ __forceinline__ float pool_window(const float* __restrict__ p, int W, int y0, int x0, int s, int type,
                                             int clamp, bool vec4) {
  float acc = type == 2 ? -INFINITY : 0.f;
  for (int r = 0; r < s; ++r) {
    const float* row = p + (long)(y0 + r) * W + x0;
    if (vec4) {
      for (int c = 0; c < s; c += 4) {
        const float4 v = *reinterpret_cast<const float4*>(row + c);
        float e[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const float x = clamp ? clamp01f(e[j]) : e[j];
          acc = type == 2 ? fmaxf(acc, x) : acc + x;
        }
      }
    } else {
      for (int c = 0; c < s; ++c) {
        const float x = clamp ? clamp01f(row[c]) : row[c];
        acc = type == 2 ? fmaxf(acc, x) : acc + x;
      }
    }
  }
  return type == 1 ? acc / (float)(s * s) : acc;
}

// pool_window for S in {4, 16} on float4 rows, NI planes at once: each batch of RB rows of every plane is loaded
// before any of it is added, so RB S/4 NI 16-byte loads are in flight together; the adds stay row-major sequential
template <int S, int NI>
__device__ __forceinline__ void pool_window_fixed(const float* const* __restrict__ p, int W, int y0, int x0, int type,
                                                  int clamp, float* out) {
  float acc[NI];
#pragma unroll
  for (int i = 0; i < NI; ++i) acc[i] = type == 2 ? -INFINITY : 0.f;
  constexpr int RB = S == 4 ? 4 : 2;   // 16 x 16 windows: 2 rows per batch keeps the kernel at <= 128 VGPRs
#pragma unroll 1
  for (int r0 = 0; r0 < S; r0 += RB) {
    float4 v[NI][RB][S / 4];
#pragma unroll
    for (int i = 0; i < NI; ++i)
#pragma unroll
      for (int r = 0; r < RB; ++r)
#pragma unroll
        for (int c = 0; c < S / 4; ++c)
          v[i][r][c] = *reinterpret_cast<const float4*>(p[i] + (long)(y0 + r0 + r) * W + x0 + 4 * c);
#pragma unroll
    for (int i = 0; i < NI; ++i)
#pragma unroll
      for (int r = 0; r < RB; ++r)
#pragma unroll
        for (int c = 0; c < S / 4; ++c) {
          const float e[4] = {v[i][r][c].x, v[i][r][c].y, v[i][r][c].z, v[i][r][c].w};
#pragma unroll
          for (int j = 0; j < 4; ++j) {
            const float x = clamp ? clamp01f(e[j]) : e[j];
            acc[i] = type == 2 ? fmaxf(acc[i], x) : acc[i] + x;
          }
        }
  }
#pragma unroll
  for (int i = 0; i < NI; ++i) out[i] = type == 1 ? acc[i] / (float)(S * S) : acc[i];
}

// NI windows at the same place of NI planes
template <int NI>
__device__ __forceinline__ void pool_windows(const float* const* __restrict__ p, int W, int y0, int x0, int s,
                                             int type, int clamp, bool vec4, float* out) {
  if (vec4 && s == 4) {
    pool_window_fixed<4, NI>(p, W, y0, x0, type, clamp, out);
  } else if (vec4 && s == 16) {
    pool_window_fixed<16, NI>(p, W, y0, x0, type, clamp, out);
  } else {
#pragma unroll
    for (int i = 0; i < NI; ++i) out[i] = pool_window(p[i], W, y0, x0, s, type, clamp, vec4);
  }
}

// the same window of the ensemble mean (sequential sum over the N members, / N, per pixel)
__device__ __forceinline__ float pool_window_mean(const float* __restrict__ p, long mstride, int N, int W, int y0,
                                                  int x0, int s, int type, int clamp) {
  float acc = type == 2 ? -INFINITY : 0.f;
  for (int r = 0; r < s; ++r)
    for (int c = 0; c < s; ++c) {
      const long o = (long)(y0 + r) * W + x0 + c;
      float m = 0.f;
      for (int n = 0; n < N; ++n) {
        const float x = p[n * mstride + o];
        m += clamp ? clamp01f(x) : x;
      }
      m = m / (float)N;
      acc = type == 2 ? fmaxf(acc, m) : acc + m;
    }
  return type == 1 ? acc / (float)(s * s) : acc;
}

// reference crps (:18-41) at one cell, in fp32 op by op like the torch expression
// (torch.distributions.Normal(0, 1): cdf = 0.5 (1 + erf(x / sqrt 2)), pdf = exp(log_prob))
__device__ __forceinline__ float crps_cell(float mean, float sd, float gt) {
  const float eps = 1e-10f;
  const float normed = (mean - gt + eps) / (sd + eps);
  const float cdf = 0.5f * (1.f + erff(normed / 1.41421356237309515f));
  const float pdf = expf(-(normed * normed) / 2.f - 0.918938533204672742f);
  return (sd + eps) * (normed * (2.f * cdf - 1.f) + 2.f * pdf - 0.564189583547756287f);
}

__global__ __launch_bounds__(kBlock) void skill_part_kernel(const float* __restrict__ pred,
                                                            const float* __restrict__ tgt, int N, int TC, int H,
                                                            int W, long planes, int clamp, int vec_ok, SkillCfg cfg,
                                                            unsigned long long* __restrict__ rows) {
  __shared__ unsigned long long cnt_sm[kBlock / 64][3 * kMaxThr];
  __shared__ double sm[16];
  int pool = 0;
  while (pool + 1 < cfg.n_pools && !((int)blockIdx.x >= cfg.blk_lo[pool] && (int)blockIdx.x < cfg.blk_hi[pool])) ++pool;
  const int type = cfg.type[pool], s = cfg.scale[pool];
  const int lb = blockIdx.x - cfg.blk_lo[pool], nb = cfg.blk_hi[pool] - cfg.blk_lo[pool];
  const int Ho = H / s, Wo = W / s;
  const long cells = planes * Ho * Wo;
  const long HW = (long)H * W;
  const bool vec4 = vec_ok && (s % 4 == 0);
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;

  unsigned cnt[3 * kMaxThr];   // per block < 2^32 cells: the host caps the tensor at 2^40 elements
#pragma unroll
  for (int j = 0; j < 3 * kMaxThr; ++j) cnt[j] = 0;
  double crps = 0.0;

  // the loop bound is block-uniform, so every lane reaches each ballot
  for (long base = (long)lb * kBlock; base < cells; base += (long)nb * kBlock) {
    const long idx = base + threadIdx.x;
    const bool active = idx < cells;
    float sp = 0.f, tg = 0.f;
    if (active) {
      const long plane = idx / ((long)Ho * Wo);
      const int rem = (int)(idx - plane * Ho * Wo);
      const int y0 = (rem / Wo) * s, x0 = (rem % Wo) * s;
      const long b = plane / TC, tc = plane - b * TC;
      const float* tp = tgt + plane * HW;
      const float* pp = pred + (b * N * TC + tc) * HW;   // member 0 of (b, tc)
      float mean, sd;
      if (N == 1) {
        const float* const planes2[2] = {tp, pp};
        float v[2];
        pool_windows<2>(planes2, W, y0, x0, s, type, clamp, vec4, v);
        tg = v[0];
        sp = mean = v[1];
        sd = 0.f;
      } else {
        pool_windows<1>(&tp, W, y0, x0, s, type, clamp, vec4, &tg);
        // counts: pool of the ensemble mean; CRPS: mean / Bessel std over the pooled members
        sp = pool_window_mean(pp, TC * HW, N, W, y0, x0, s, type, clamp);
        float msum = 0.f;
        double wm = 0.0, m2 = 0.0;
        for (int n = 0; n < N; ++n) {
          const float* pm = pp + n * TC * HW;
          float v;
          pool_windows<1>(&pm, W, y0, x0, s, type, clamp, vec4, &v);
          msum += v;
          const double d = (double)v - wm;
          wm += d / (n + 1);
          m2 += d * ((double)v - wm);
        }
        mean = msum / (float)N;
        sd = (float)sqrt(m2 / (N - 1));
      }
      crps += (double)crps_cell(mean, sd, tg);
    }
#pragma unroll
    for (int k = 0; k < kMaxThr; ++k) {
      if (k < cfg.n_thr) {
        const unsigned long long mp = __ballot(active && sp >= cfg.thr[k]);
        const unsigned long long mt = __ballot(active && tg >= cfg.thr[k]);
        cnt[3 * k] += __popcll(mp & mt);
        cnt[3 * k + 1] += __popcll(~mp & mt);
        cnt[3 * k + 2] += __popcll(mp & ~mt);
      }
    }
  }

  if (lane == 0) {
#pragma unroll
    for (int j = 0; j < 3 * kMaxThr; ++j) cnt_sm[wv][j] = cnt[j];
  }
  const double cs = block_sum(crps, sm);   // contains the barrier that publishes cnt_sm
  // column-major partial rows: value j of block b at rows[j * gridDim.x + b]
  if (threadIdx.x < 3 * kMaxThr) {
    unsigned long long t = 0;
    for (int w = 0; w < kBlock / 64; ++w) t += cnt_sm[w][threadIdx.x];
    rows[(long)threadIdx.x * gridDim.x + blockIdx.x] = t;
  }
  if (threadIdx.x == 0) rows[(long)3 * kMaxThr * gridDim.x + blockIdx.x] = __double_as_longlong(cs);
}

__device__ __forceinline__ unsigned long long wave_sum_u64(unsigned long long v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// one block per pool: fixed-order reduction of the pool's partial rows into
// out[pool] = [tp, fn, fp] x n_thr, CRPS sum (double bits), pooled cell count
__global__ __launch_bounds__(kFinal) void skill_finalize_kernel(const unsigned long long* __restrict__ rows, int nrows,
                                                                long planes, int H, int W, SkillCfg cfg,
                                                                long long* __restrict__ out) {
  __shared__ unsigned long long red[kFinal / 64][3 * kMaxThr];
  __shared__ double sm[16];
  const int pool = blockIdx.x;
  const int r0 = cfg.blk_lo[pool], r1 = cfg.blk_hi[pool];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int nc = 3 * cfg.n_thr;
  unsigned long long acc[3 * kMaxThr];
#pragma unroll
  for (int j = 0; j < 3 * kMaxThr; ++j) acc[j] = 0;
  double cs = 0.0;
  for (int r = r0 + threadIdx.x; r < r1; r += kFinal) {   // every column of a row in flight at once
#pragma unroll
    for (int j = 0; j < 3 * kMaxThr; ++j) acc[j] += rows[(long)j * nrows + r];
    cs += __longlong_as_double(rows[(long)3 * kMaxThr * nrows + r]);
  }
#pragma unroll
  for (int j = 0; j < 3 * kMaxThr; ++j) {
    const unsigned long long v = wave_sum_u64(acc[j]);
    if (lane == 0) red[wv][j] = v;
  }
  const double tot = block_sum(cs, sm);
  const int stride = nc + 2;
  if (threadIdx.x < nc) {
    unsigned long long t = 0;
    for (int w = 0; w < kFinal / 64; ++w) t += red[w][threadIdx.x];
    out[(long)pool * stride + threadIdx.x] = (long long)t;
  }
  if (threadIdx.x == 0) {
    const int s = cfg.scale[pool];
    out[(long)pool * stride + nc] = __double_as_longlong(tot);
    out[(long)pool * stride + nc + 1] = (long long)(planes * (H / s) * (W / s));
  }
}

__global__ __launch_bounds__(kBlock) void ensemble_mean_kernel(const float* __restrict__ pred, float* __restrict__ out,
                                                               long outer, int N, long inner, int clamp) {
  const long total = outer * inner;
  for (long i = (long)blockIdx.x * kBlock + threadIdx.x; i < total; i += (long)gridDim.x * kBlock) {
    const long o = i / inner, k = i - o * inner;
    const float* p = pred + o * N * inner + k;
    float m = 0.f;
    for (int n = 0; n < N; ++n) {
      const float x = p[n * inner];
      m += clamp ? clamp01f(x) : x;
    }
    out[i] = m / (float)N;
  }
}

}  // namespace

extern "C" {

int wfae_skill_scores(const float* pred, const float* target, int64_t* out, int B, int N, int TC, int H, int W,
                      const float* thresholds, int n_thr, const int* pool_types, const int* pool_scales, int n_pools,
                      int clamp01, void* ws, size_t ws_bytes, wfae_stream_t stream) {
  WFAE_REQUIRE(pred && target && out, WFAE_ERR_NULL_POINTER, "skill_scores: null pointer");
  WFAE_REQUIRE(n_pools >= 1 && n_pools <= kMaxPools && pool_types && pool_scales, WFAE_ERR_BAD_SHAPE,
               "skill_scores: n_pools %d not in [1, %d]", n_pools, kMaxPools);
  WFAE_REQUIRE(n_thr >= 0 && n_thr <= kMaxThr && (n_thr == 0 || thresholds), WFAE_ERR_BAD_SHAPE,
               "skill_scores: n_thr %d not in [0, %d]", n_thr, kMaxThr);
  WFAE_REQUIRE(B > 0 && N > 0 && TC > 0 && H > 0 && W > 0, WFAE_ERR_BAD_SHAPE, "skill_scores: bad shape");
  const long planes = (long)B * TC;
  WFAE_REQUIRE(planes * N <= (1L << 40) / ((long)H * W), WFAE_ERR_BAD_SHAPE, "skill_scores: tensor too large");
  SkillCfg cfg{};
  cfg.n_pools = n_pools;
  cfg.n_thr = n_thr;
  for (int k = 0; k < n_thr; ++k) cfg.thr[k] = thresholds[k];
  int nb[kMaxPools];
  for (int p = 0; p < n_pools; ++p) {
    const int t = pool_types[p], s = t == 0 ? 1 : pool_scales[p];
    WFAE_REQUIRE(t >= 0 && t <= 2, WFAE_ERR_BAD_SHAPE, "skill_scores: pool type %d (0 none, 1 avg, 2 max)", t);
    WFAE_REQUIRE(s >= 1 && s <= H && s <= W, WFAE_ERR_BAD_SHAPE, "skill_scores: pool scale %d outside [1, min(H, W)]",
                 pool_scales[p]);
    cfg.type[p] = t;
    cfg.scale[p] = s;
    const long cells = planes * (H / s) * (W / s);
    const long want = (cells + kBlock - 1) / kBlock;
    nb[p] = (int)(want < kMaxBlocksPerPool ? want : kMaxBlocksPerPool);
  }
  // the pools with the longest per-lane windows take the front of the grid, so they start first
  int nblk = 0;
  for (int done = 0; done < n_pools; ++done) {
    int q = -1;
    for (int p = 0; p < n_pools; ++p)
      if (cfg.scale[p] > 0 && (q < 0 || cfg.scale[p] > cfg.scale[q])) q = p;
    cfg.blk_lo[q] = nblk;
    nblk += nb[q];
    cfg.blk_hi[q] = nblk;
    cfg.scale[q] = -cfg.scale[q];   // taken
  }
  for (int p = 0; p < n_pools; ++p) cfg.scale[p] = -cfg.scale[p];
  const size_t need = (size_t)nblk * kRow * sizeof(unsigned long long);
  WFAE_REQUIRE(ws && ws_bytes >= need, WFAE_ERR_WORKSPACE, "skill_scores: workspace %zu < %zu", ws_bytes, need);
  // 16-byte row loads when every window row starts on a 16-byte boundary
  const int vec_ok = (W % 4 == 0) && ((uintptr_t)pred % 16 == 0) && ((uintptr_t)target % 16 == 0);
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(skill_part_kernel, dim3(nblk), dim3(kBlock), 0, st, pred, target, N, TC, H, W, planes, clamp01,
                     vec_ok, cfg, (unsigned long long*)ws);
  int rc = check_launch("skill_part");
  if (rc) return rc;
  hipLaunchKernelGGL(skill_finalize_kernel, dim3(n_pools), dim3(kFinal), 0, st, (const unsigned long long*)ws, nblk,
                     planes, H, W, cfg, (long long*)out);
  return check_launch("skill_finalize");
}

int wfae_ensemble_mean(const float* pred, float* out, int64_t outer, int N, int64_t inner, int clamp01,
                       wfae_stream_t stream) {
  WFAE_REQUIRE(pred && out, WFAE_ERR_NULL_POINTER, "ensemble_mean: null pointer");
  WFAE_REQUIRE(outer > 0 && N > 0 && inner > 0 && outer * N <= (1L << 40) / inner, WFAE_ERR_BAD_SHAPE,
               "ensemble_mean: bad shape");
  const long total = outer * inner;
  long g = (total + kBlock - 1) / kBlock;
  if (g > 2048) g = 2048;
  hipLaunchKernelGGL(ensemble_mean_kernel, dim3((int)g), dim3(kBlock), 0, (hipStream_t)stream, pred, out, (long)outer,
                     N, (long)inner, clamp01);
  return check_launch("ensemble_mean");
}

}  // extern "C"
