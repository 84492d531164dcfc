// dlinear.hip — kernels of the DLinear latent forecasters (reference
// experiments/v1_experiments/pretrained_ae_dlinear_{sevir,ind,indc_indp}/train.py:22-100): the moving-average
// decomposition with replicate padding (`moving_avg`, `series_decomp`), the seasonal + trend linear maps with shared
// (P x L) or per-column (M x P x L) weights, their gradients, and the layout-free target / forecast epilogues.
//
// Generic shape: the latent sequence is v (B, R, M) — R rows per batch element, M columns (latent scalars or latent
// pixels).  The predictor reads rows [0, L) (optionally differenced against the last input frame: row r minus row
// L - cf + r % cf, the reference's `inp - inp_t`), and writes y (B, P, M).  Columns are the coalesced axis of every
// global access.
//
// Row-mapped kernels (forward, per-column weight gradient): one thread per weight row r = m * P + p, so the 256 threads
// of a block sweep one contiguous 256 L-float stretch of the (M, P, L) weight tensor (each weight is read once per step,
// the batch loop runs inside the thread); the block's few columns of seasonal / trend are formed in LDS.  Shared weights:
// block partials over 64-column chunks + a finalize pass in a fixed order.  No atomics anywhere: repeated calls give
// identical bits.
#include "common.h"

using namespace wfae;

namespace {

constexpr int kThreads = 256;
constexpr int kBmax = 8;           // batch elements per LDS chunk / per-thread accumulators
constexpr int kSharedCols = 64;    // column chunk of the shared-weight gradient partials
constexpr int kSharedStride = kSharedCols + 1;   // odd LDS row stride: lanes that differ in (p, l) hit distinct banks
constexpr int kEntMax = 24;        // shared gradient entries per thread: 2 P L + P <= 24 * 256
constexpr size_t kLdsMax = 64 * 1024;

struct DlShape {
  int B, R, M, L, P, K, diff, cf;
};

__device__ __forceinline__ float xval(const float* __restrict__ v, const DlShape& s, int b, int l, int m) {
  const long base = (long)b * s.R;
  float x = v[(base + l) * s.M + m];
  if (s.diff) x -= v[(base + s.L - s.cf + l % s.cf) * s.M + m];
  return x;
}

// S / T [bb][l][c] (row stride ncs) <- seasonal / trend of batch elements b0 .. b0+bc-1, columns m0 .. m0+nc-1
// (columns past M are zero).  trend = sum of the K replicate-padded neighbours / K (AvgPool1d order), seasonal = x - trend.
__device__ void stage_decomp(const float* __restrict__ v, float* S, float* T, int b0, int bc, int m0, int nc, int ncs,
                             const DlShape& s) {
  const int L = s.L, n = bc * L * nc;
  for (int i = threadIdx.x; i < n; i += blockDim.x) {
    const int c = i % nc, t = i / nc, l = t % L, bb = t / L;
    const int m = m0 + c;
    S[(bb * L + l) * ncs + c] = m < s.M ? xval(v, s, b0 + bb, l, m) : 0.f;
  }
  __syncthreads();
  const int h = (s.K - 1) / 2;
  for (int i = threadIdx.x; i < n; i += blockDim.x) {
    const int c = i % nc, t = i / nc, l = t % L, bb = t / L;
    float acc = 0.f;
    for (int k = 0; k < s.K; ++k) {
      const int j = min(max(l + k - h, 0), L - 1);
      acc += S[(bb * L + j) * ncs + c];
    }
    T[(bb * L + l) * ncs + c] = acc / (float)s.K;
  }
  __syncthreads();
  for (int i = threadIdx.x; i < n; i += blockDim.x) {
    const int c = i % nc, t = i / nc, l = t % L, bb = t / L;
    S[(bb * L + l) * ncs + c] -= T[(bb * L + l) * ncs + c];
  }
  __syncthreads();
}

// WGRAD = false: y[b,p,m] = Ws[w] . s[b,:,m] + bs[w] + Wt[w] . t[b,:,m] + bt[w], w = m*P+p (individual) or p (shared).
// WGRAD = true (individual only): dWs[m,p,:] = sum_b dy[b,p,m] s[b,:,m], dWt likewise with t, dbs = dbt = sum_b dy.
template <bool WGRAD>
__global__ __launch_bounds__(kThreads) void dl_rows_kernel(const float* __restrict__ v, const float* __restrict__ dy,
                                                           const float* __restrict__ ws, const float* __restrict__ bs,
                                                           const float* __restrict__ wt, const float* __restrict__ bt,
                                                           float* __restrict__ y, float* __restrict__ dws,
                                                           float* __restrict__ dbs, float* __restrict__ dwt,
                                                           float* __restrict__ dbt, DlShape s, int individual,
                                                           int bcmax, int ncs) {
  extern __shared__ float sm[];
  const int L = s.L, P = s.P, M = s.M;
  const long rows = (long)M * P;
  const long r0 = (long)blockIdx.x * kThreads;
  const long rlast = min(r0 + kThreads - 1, rows - 1);
  const int m0 = (int)(r0 / P);
  const int nc = (int)(rlast / P) - m0 + 1;
  float* S = sm;
  float* T = S + bcmax * L * ncs;
  float* Y = T + bcmax * L * ncs;   // [bb][p][c]: output tile (forward) or dy tile (weight gradient)
  const long r = r0 + threadIdx.x;
  const bool act = r < rows;
  const int m = act ? (int)(r / P) : m0, p = act ? (int)(r % P) : 0, c = m - m0;
  const long wrow = individual ? r : p;
  for (int b0 = 0; b0 < s.B; b0 += bcmax) {
    const int bc = min(bcmax, s.B - b0);
    if (WGRAD) {
      for (int i = threadIdx.x; i < bc * P * nc; i += blockDim.x) {
        const int cc = i % nc, t = i / nc, pp = t % P, bb = t / P;
        Y[(bb * P + pp) * ncs + cc] = dy[((long)(b0 + bb) * P + pp) * M + m0 + cc];
      }
    }
    stage_decomp(v, S, T, b0, bc, m0, nc, ncs, s);
    if (!WGRAD) {
      float acc[kBmax];
      const float b0v = act ? bs[wrow] + bt[wrow] : 0.f;
#pragma unroll
      for (int bb = 0; bb < kBmax; ++bb) acc[bb] = b0v;
      if (act) {
        const float* __restrict__ wsr = ws + wrow * L;
        const float* __restrict__ wtr = wt + wrow * L;
        for (int l = 0; l < L; ++l) {
          const float a = wsr[l], e = wtr[l];
#pragma unroll
          for (int bb = 0; bb < kBmax; ++bb)
            if (bb < bc) acc[bb] += a * S[(bb * L + l) * ncs + c] + e * T[(bb * L + l) * ncs + c];
        }
#pragma unroll
        for (int bb = 0; bb < kBmax; ++bb)
          if (bb < bc) Y[(bb * P + p) * ncs + c] = acc[bb];
      }
      __syncthreads();
      // coalesced store of the rows this block owns (edge columns are shared with the neighbouring blocks)
      for (int i = threadIdx.x; i < bc * P * nc; i += blockDim.x) {
        const int cc = i % nc, t = i / nc, pp = t % P, bb = t / P;
        const long rr = (long)(m0 + cc) * P + pp;
        if (rr >= r0 && rr <= rlast) y[((long)(b0 + bb) * P + pp) * M + m0 + cc] = Y[(bb * P + pp) * ncs + cc];
      }
    } else if (act) {
      float g[kBmax];
      float gb = 0.f;
#pragma unroll
      for (int bb = 0; bb < kBmax; ++bb) {
        g[bb] = bb < bc ? Y[(bb * P + p) * ncs + c] : 0.f;
        gb += g[bb];
      }
      float* __restrict__ dwsr = dws + r * L;
      float* __restrict__ dwtr = dwt + r * L;
      for (int l = 0; l < L; ++l) {
        float gs = 0.f, gt = 0.f;
#pragma unroll
        for (int bb = 0; bb < kBmax; ++bb)
          if (bb < bc) {
            gs += g[bb] * S[(bb * L + l) * ncs + c];
            gt += g[bb] * T[(bb * L + l) * ncs + c];
          }
        if (b0 == 0) {
          dwsr[l] = gs;
          dwtr[l] = gt;
        } else {
          dwsr[l] += gs;
          dwtr[l] += gt;
        }
      }
      if (b0 == 0) {
        dbs[r] = gb;
        dbt[r] = gb;
      } else {
        dbs[r] += gb;
        dbt[r] += gb;
      }
    }
    __syncthreads();   // the next chunk overwrites the LDS tiles
  }
}

// shared weights: part[blk][e], e < P L: sum over the block's 64 columns and all b of dy[b,p,m] s[b,l,m]
// (e = p L + l); P L <= e < 2 P L: the same with t; 2 P L <= e: sum of dy[b,p,m] (p = e - 2 P L)
__global__ __launch_bounds__(kThreads) void dl_wgrad_shared_part_kernel(const float* __restrict__ v,
                                                                        const float* __restrict__ dy,
                                                                        float* __restrict__ part, DlShape s) {
  extern __shared__ float sm[];
  const int L = s.L, P = s.P, M = s.M, PL = P * L, E = 2 * PL + P;
  const int m0 = blockIdx.x * kSharedCols, nc = min(kSharedCols, M - m0);
  float* S = sm;
  float* T = S + L * kSharedStride;
  float* G = T + L * kSharedStride;
  float acc[kEntMax];
#pragma unroll
  for (int j = 0; j < kEntMax; ++j) acc[j] = 0.f;
  for (int b = 0; b < s.B; ++b) {
    for (int i = threadIdx.x; i < P * kSharedCols; i += blockDim.x) {
      const int cc = i % kSharedCols, pp = i / kSharedCols;
      G[pp * kSharedStride + cc] = cc < nc ? dy[((long)b * P + pp) * M + m0 + cc] : 0.f;
    }
    stage_decomp(v, S, T, b, 1, m0, kSharedCols, kSharedStride, s);
#pragma unroll
    for (int j = 0; j < kEntMax; ++j) {
      const int e = threadIdx.x + j * kThreads;
      if (e < E) {
        const float* a;
        const float* q;
        if (e < PL) {
          a = G + (e / L) * kSharedStride;
          q = S + (e % L) * kSharedStride;
        } else if (e < 2 * PL) {
          a = G + ((e - PL) / L) * kSharedStride;
          q = T + ((e - PL) % L) * kSharedStride;
        } else {
          a = G + (e - 2 * PL) * kSharedStride;
          q = nullptr;
        }
        float sum = 0.f;
        if (q) {
          for (int cc = 0; cc < nc; ++cc) sum += a[cc] * q[cc];
        } else {
          for (int cc = 0; cc < nc; ++cc) sum += a[cc];
        }
        acc[j] += sum;
      }
    }
    __syncthreads();
  }
#pragma unroll
  for (int j = 0; j < kEntMax; ++j) {
    const int e = threadIdx.x + j * kThreads;
    if (e < E) part[(long)blockIdx.x * E + e] = acc[j];
  }
}

__global__ void dl_wgrad_shared_final_kernel(const float* __restrict__ part, int nblk, int P, int L,
                                             float* __restrict__ dws, float* __restrict__ dbs,
                                             float* __restrict__ dwt, float* __restrict__ dbt) {
  const int PL = P * L, E = 2 * PL + P;
  const int e = blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= E) return;
  double sum = 0.0;
  for (int k = 0; k < nblk; ++k) sum += (double)part[(long)k * E + e];
  const float r = (float)sum;
  if (e < PL) dws[e] = r;
  else if (e < 2 * PL) dwt[e - PL] = r;
  else {
    dbs[e - 2 * PL] = r;
    dbt[e - 2 * PL] = r;
  }
}

// gs / gt (B, L, M) = Ws^T dy / Wt^T dy per column (the gradients w.r.t. seasonal and trend)
__global__ __launch_bounds__(kThreads) void dl_dst_kernel(const float* __restrict__ dy, const float* __restrict__ ws,
                                                          const float* __restrict__ wt, float* __restrict__ gs,
                                                          float* __restrict__ gt, int B, int M, int L, int P,
                                                          int individual) {
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= (long)B * M) return;
  const int b = (int)(i / M), m = (int)(i % M);
  const long wb = individual ? (long)m * P * L : 0;
  const float* __restrict__ g = dy + (long)b * P * M + m;
  for (int l = 0; l < L; ++l) {
    float a = 0.f, e = 0.f;
    for (int p = 0; p < P; ++p) {
      const float d = g[(long)p * M];
      a += ws[wb + (long)p * L + l] * d;
      e += wt[wb + (long)p * L + l] * d;
    }
    gs[((long)b * L + l) * M + m] = a;
    gt[((long)b * L + l) * M + m] = e;
  }
}

// adjoint of (x -> seasonal, trend) at row l of one column: gs_l + sum_j cnt(j, l) (gt_j - gs_j) / K, cnt(j, l) the
// number of window taps of output row j that the replicate padding maps onto input row l
__device__ __forceinline__ float decomp_adj(const float* __restrict__ gs, const float* __restrict__ gt, long stride,
                                            int l, int L, int K) {
  const int h = (K - 1) / 2;
  float acc = 0.f;
  for (int j = max(0, l - h); j <= min(L - 1, l + h); ++j) {
    int cnt;
    if (L == 1) cnt = K;
    else if (l == 0) cnt = h - j + 1;
    else if (l == L - 1) cnt = j + h - L + 2;
    else cnt = 1;
    acc += (float)cnt * (gt[j * stride] - gs[j * stride]);
  }
  return gs[l * stride] + acc / (float)K;
}

// dx (B, R, M): rows < L the decomposition adjoint, minus (diff) the sum over the rows each last-frame row was
// subtracted from; rows >= L zero
__global__ __launch_bounds__(kThreads) void dl_decomp_bwd_kernel(const float* __restrict__ gs,
                                                                 const float* __restrict__ gt, float* __restrict__ dx,
                                                                 DlShape s) {
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= (long)s.B * s.M) return;
  const int b = (int)(i / s.M), m = (int)(i % s.M);
  const float* __restrict__ a = gs + (long)b * s.L * s.M + m;
  const float* __restrict__ e = gt + (long)b * s.L * s.M + m;
  for (int q = 0; q < s.R; ++q) {
    float val = 0.f;
    if (q < s.L) {
      val = decomp_adj(a, e, s.M, q, s.L, s.K);
      if (s.diff && q >= s.L - s.cf)
        for (int r = q % s.cf; r < s.L; r += s.cf) val -= decomp_adj(a, e, s.M, r, s.L, s.K);
    }
    dx[((long)b * s.R + q) * s.M + m] = val;
  }
}

// series_decomp of x (B, L, M) along L: seasonal, trend
__global__ __launch_bounds__(kThreads) void dl_decomp_fwd_kernel(const float* __restrict__ x, float* __restrict__ sea,
                                                                 float* __restrict__ tr, int B, int L, int M, int K) {
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= (long)B * M) return;
  const int b = (int)(i / M), m = (int)(i % M);
  const long base = (long)b * L * M + m;
  const int h = (K - 1) / 2;
  for (int l = 0; l < L; ++l) {
    float acc = 0.f;
    for (int k = 0; k < K; ++k) acc += x[base + (long)min(max(l + k - h, 0), L - 1) * M];
    const float t = acc / (float)K;
    tr[base + (long)l * M] = t;
    sea[base + (long)l * M] = x[base + (long)l * M] - t;
  }
}

// mode 0 (target): out[b,p,m] = v[b, L+p, m] - v[b, L-cf+p%cf, m]; mode 1 (forecast): out = a[b,p,m] + v[b, L-cf+p%cf, m]
__global__ __launch_bounds__(kThreads) void dl_frames_kernel(const float* __restrict__ a, const float* __restrict__ v,
                                                             float* __restrict__ out, int B, int R, int M, int L, int P,
                                                             int cf, int mode) {
  const long n = (long)B * P * M;
  const long stride = (long)gridDim.x * blockDim.x;
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
    const int m = (int)(i % M);
    const long t = i / M;
    const int p = (int)(t % P), b = (int)(t / P);
    const long base = (long)b * R;
    const float last = v[(base + L - cf + p % cf) * M + m];
    out[i] = mode == 0 ? v[(base + L + p) * M + m] - last : a[i] + last;
  }
}

int check_shape(const char* what, int B, int R, int M, int L, int P, int K, int diff, int cf) {
  WFAE_REQUIRE(B > 0 && M > 0 && L > 0 && P > 0 && R >= L, WFAE_ERR_BAD_SHAPE,
               "%s: bad shape B=%d R=%d M=%d L=%d P=%d", what, B, R, M, L, P);
  WFAE_REQUIRE(K >= 1 && K % 2 == 1, WFAE_ERR_BAD_SHAPE,
               "%s: kernel_size must be odd and >= 1 (got %d): an even window changes the sequence length", what, K);
  WFAE_REQUIRE(!diff || (cf >= 1 && cf <= L && L % cf == 0), WFAE_ERR_BAD_SHAPE,
               "%s: differencing needs L (%d) a multiple of cf (%d)", what, L, cf);
  return 0;
}

// LDS of the row-mapped kernel for a batch chunk of bc: S, T (bc L ncs each) + the output / dy tile (bc P ncs)
size_t rows_lds(int bc, int L, int P, int ncs) { return (size_t)bc * (2 * L + P) * ncs * sizeof(float); }

int rows_plan(const char* what, int B, int L, int P, int* bcmax, int* ncs) {
  *ncs = (kThreads - 1) / P + 2;   // distinct columns among 256 consecutive rows m*P+p
  int bc = B < kBmax ? B : kBmax;
  while (bc > 1 && rows_lds(bc, L, P, *ncs) > kLdsMax) --bc;
  WFAE_REQUIRE(rows_lds(bc, L, P, *ncs) <= kLdsMax, WFAE_ERR_UNSUPPORTED,
               "%s: L=%d, P=%d need %zu bytes of LDS per batch element", what, L, P, rows_lds(1, L, P, *ncs));
  *bcmax = bc;
  return 0;
}

}  // namespace

extern "C" {

int wfae_dlinear_fwd(const float* v, const float* w_seasonal, const float* b_seasonal, const float* w_trend,
                     const float* b_trend, float* y, int B, int R, int M, int L, int P, int K, int individual, int diff,
                     int cf, wfae_stream_t stream) {
  WFAE_REQUIRE(v && w_seasonal && b_seasonal && w_trend && b_trend && y, WFAE_ERR_NULL_POINTER,
               "dlinear_fwd: null pointer");
  int rc = check_shape("dlinear_fwd", B, R, M, L, P, K, diff, cf);
  if (rc) return rc;
  int bcmax, ncs;
  if ((rc = rows_plan("dlinear_fwd", B, L, P, &bcmax, &ncs))) return rc;
  const DlShape s{B, R, M, L, P, K, diff, cf};
  const size_t lds = rows_lds(bcmax, L, P, ncs);
  hipLaunchKernelGGL(dl_rows_kernel<false>, dim3(cdiv((int64_t)M * P, kThreads)), dim3(kThreads), lds,
                     (hipStream_t)stream, v, nullptr, w_seasonal, b_seasonal, w_trend, b_trend, y, nullptr, nullptr,
                     nullptr, nullptr, s, individual, bcmax, ncs);
  return check_launch("dlinear_fwd");
}

int wfae_dlinear_bwd_weight(const float* v, const float* dy, float* dw_seasonal, float* db_seasonal, float* dw_trend,
                            float* db_trend, int B, int R, int M, int L, int P, int K, int individual, int diff, int cf,
                            void* ws, size_t ws_bytes, wfae_stream_t stream) {
  WFAE_REQUIRE(v && dy && dw_seasonal && db_seasonal && dw_trend && db_trend, WFAE_ERR_NULL_POINTER,
               "dlinear_bwd_weight: null pointer");
  int rc = check_shape("dlinear_bwd_weight", B, R, M, L, P, K, diff, cf);
  if (rc) return rc;
  const DlShape s{B, R, M, L, P, K, diff, cf};
  hipStream_t st = (hipStream_t)stream;
  if (individual) {
    int bcmax, ncs;
    if ((rc = rows_plan("dlinear_bwd_weight", B, L, P, &bcmax, &ncs))) return rc;
    hipLaunchKernelGGL(dl_rows_kernel<true>, dim3(cdiv((int64_t)M * P, kThreads)), dim3(kThreads),
                       rows_lds(bcmax, L, P, ncs), st, v, dy, nullptr, nullptr, nullptr, nullptr, nullptr, dw_seasonal,
                       db_seasonal, dw_trend, db_trend, s, 1, bcmax, ncs);
    return check_launch("dlinear_bwd_weight");
  }
  const int E = 2 * P * L + P;
  WFAE_REQUIRE(E <= kEntMax * kThreads, WFAE_ERR_UNSUPPORTED,
               "dlinear_bwd_weight: shared weights need 2 P L + P <= %d (P=%d, L=%d)", kEntMax * kThreads, P, L);
  const size_t lds = (size_t)(2 * L + P) * kSharedStride * sizeof(float);
  WFAE_REQUIRE(lds <= kLdsMax, WFAE_ERR_UNSUPPORTED, "dlinear_bwd_weight: L=%d, P=%d too large for LDS", L, P);
  const int nblk = cdiv(M, kSharedCols);
  WFAE_REQUIRE(ws && ws_bytes >= (size_t)nblk * E * sizeof(float), WFAE_ERR_WORKSPACE,
               "dlinear_bwd_weight: workspace too small (%zu < %zu)", ws_bytes, (size_t)nblk * E * sizeof(float));
  hipLaunchKernelGGL(dl_wgrad_shared_part_kernel, dim3(nblk), dim3(kThreads), lds, st, v, dy, (float*)ws, s);
  if ((rc = check_launch("dlinear_bwd_weight_part"))) return rc;
  hipLaunchKernelGGL(dl_wgrad_shared_final_kernel, dim3(cdiv(E, kThreads)), dim3(kThreads), 0, st, (const float*)ws,
                     nblk, P, L, dw_seasonal, db_seasonal, dw_trend, db_trend);
  return check_launch("dlinear_bwd_weight_final");
}

int wfae_dlinear_bwd_data(const float* dy, const float* w_seasonal, const float* w_trend, float* dv, int B, int R,
                          int M, int L, int P, int K, int individual, int diff, int cf, void* ws, size_t ws_bytes,
                          wfae_stream_t stream) {
  WFAE_REQUIRE(dy && w_seasonal && w_trend && dv, WFAE_ERR_NULL_POINTER, "dlinear_bwd_data: null pointer");
  int rc = check_shape("dlinear_bwd_data", B, R, M, L, P, K, diff, cf);
  if (rc) return rc;
  const size_t need = (size_t)2 * B * L * M * sizeof(float);
  WFAE_REQUIRE(ws && ws_bytes >= need, WFAE_ERR_WORKSPACE, "dlinear_bwd_data: workspace too small (%zu < %zu)",
               ws_bytes, need);
  float* gs = (float*)ws;
  float* gt = gs + (size_t)B * L * M;
  hipStream_t st = (hipStream_t)stream;
  const int grid = cdiv((int64_t)B * M, kThreads);
  hipLaunchKernelGGL(dl_dst_kernel, dim3(grid), dim3(kThreads), 0, st, dy, w_seasonal, w_trend, gs, gt, B, M, L, P,
                     individual);
  if ((rc = check_launch("dlinear_bwd_data_dst"))) return rc;
  const DlShape s{B, R, M, L, P, K, diff, cf};
  hipLaunchKernelGGL(dl_decomp_bwd_kernel, dim3(grid), dim3(kThreads), 0, st, gs, gt, dv, s);
  return check_launch("dlinear_bwd_data");
}

int wfae_series_decomp_fwd(const float* x, float* seasonal, float* trend, int B, int L, int M, int K,
                           wfae_stream_t stream) {
  WFAE_REQUIRE(x && seasonal && trend, WFAE_ERR_NULL_POINTER, "series_decomp_fwd: null pointer");
  int rc = check_shape("series_decomp_fwd", B, L, M, L, 1, K, 0, 1);
  if (rc) return rc;
  hipLaunchKernelGGL(dl_decomp_fwd_kernel, dim3(cdiv((int64_t)B * M, kThreads)), dim3(kThreads), 0,
                     (hipStream_t)stream, x, seasonal, trend, B, L, M, K);
  return check_launch("series_decomp_fwd");
}

int wfae_series_decomp_bwd(const float* dseasonal, const float* dtrend, float* dx, int B, int L, int M, int K,
                           wfae_stream_t stream) {
  WFAE_REQUIRE(dseasonal && dtrend && dx, WFAE_ERR_NULL_POINTER, "series_decomp_bwd: null pointer");
  int rc = check_shape("series_decomp_bwd", B, L, M, L, 1, K, 0, 1);
  if (rc) return rc;
  const DlShape s{B, L, M, L, 1, K, 0, 1};
  hipLaunchKernelGGL(dl_decomp_bwd_kernel, dim3(cdiv((int64_t)B * M, kThreads)), dim3(kThreads), 0,
                     (hipStream_t)stream, dseasonal, dtrend, dx, s);
  return check_launch("series_decomp_bwd");
}

int wfae_dlinear_frames(const float* a, const float* v, float* out, int B, int R, int M, int L, int P, int cf, int mode,
                        wfae_stream_t stream) {
  WFAE_REQUIRE(v && out && (mode == 0 || a), WFAE_ERR_NULL_POINTER, "dlinear_frames: null pointer");
  WFAE_REQUIRE(mode == 0 || mode == 1, WFAE_ERR_BAD_SHAPE, "dlinear_frames: mode %d", mode);
  WFAE_REQUIRE(B > 0 && M > 0 && L > 0 && P > 0 && cf >= 1 && cf <= L && L % cf == 0 && R >= (mode == 0 ? L + P : L),
               WFAE_ERR_BAD_SHAPE, "dlinear_frames: bad shape B=%d R=%d M=%d L=%d P=%d cf=%d", B, R, M, L, P, cf);
  const int64_t n = (int64_t)B * P * M;
  int blocks = cdiv(n, kThreads * 4);
  if (blocks > 8192) blocks = 8192;
  hipLaunchKernelGGL(dl_frames_kernel, dim3(blocks), dim3(kThreads), 0, (hipStream_t)stream, a, v, out, B, R, M, L, P,
                     cf, mode);
  return check_launch("dlinear_frames");
}

}  // extern "C"
