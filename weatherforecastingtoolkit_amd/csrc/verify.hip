// verify.hip — forecast verification per lead time: up to 4 fields (forecast, persistence, reconstruction, ...) scored
// against one target in one pass.  Per lead and field: the contingency counts behind CSI / HSS at up to 8 thresholds
// (`value >= threshold` in fp32, as _hit_miss_fa_cn of the reference's pipeline/metrics.py and skill.hip form them)
// and the fp64 sums of e^2 and |e|, e = (double)field - (double)target.
//
// A field is (pointer, sample stride, lead stride) in elements; a lead stride of 0 is the same frame at every lead
// (persistence: the last input frame as a view of the loader batch).  The S pixels of one frame are contiguous.  Nothing
// is copied: the kernel reads the views.  16-byte loads when S % 4 == 0 and every base and stride is 16-byte aligned,
// dword loads otherwise.
//
// Grid: block b serves lead b % P and cell chunk b / P, so the blocks that share a lead-stride-0 frame run side by side
// and find it in the L2.  Each lane counts its own cells (field events, hits, target events: misses and false alarms are
// differences), the target's event bits are formed once per cell for all fields.  Blocks write partial rows; the finalize
// kernel adds the fp64 partials of a (lead, field) in ascending block order — no atomics, the same bits on every run.
#include "common.h"

using namespace wfae;

namespace {

constexpr int kBlock = 256;
constexpr int kMaxF = 4, kMaxThr = 8;
constexpr int kMaxChunks = 256;        // chunks per lead; the finalize block has one thread per chunk
constexpr int kCellsPerChunkTrip = 1024;

struct VerifyCfg {
  const float* field[kMaxF];
  long fb[kMaxF], fl[kMaxF];   // elements between samples / leads of each field
  const float* tgt;
  long tb, tl;
  long S;
  int F, B, P, n_thr, clamp, nchunk;
  float thr[kMaxThr];           // [n_thr, kMaxThr): +inf, which no finite value reaches
};

__device__ __forceinline__ float clamp01f(float v) { return fminf(fmaxf(v, 0.f), 1.f); }

__device__ __forceinline__ unsigned wave_sum_u32(unsigned v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

template <int V>
__device__ __forceinline__ void load_cells(const float* __restrict__ p, float (&v)[V]) {
  if constexpr (V == 4) {
    const float4 r = *reinterpret_cast<const float4*>(p);
    v[0] = r.x; v[1] = r.y; v[2] = r.z; v[3] = r.w;
  } else {
    v[0] = *p;
  }
}

// partial row of block b, column-major in the workspace (value j at rows[j * gridDim.x + b]):
// per field [tp, fn, fp] x n_thr, then per field the bits of sum e^2 and sum |e|
// NT: thresholds compared per cell (n_thr rounded up to 6 or 8; the padding thresholds are +inf and count nothing)
template <int V, int F, int NT>
__global__ __launch_bounds__(kBlock) void verify_part_kernel(VerifyCfg c, unsigned long long* __restrict__ rows) {
  __shared__ unsigned long long cnt_sm[kBlock / 64][kMaxF * 3 * kMaxThr];
  __shared__ double sm[16];
  const int p = blockIdx.x % c.P, chunk = blockIdx.x / c.P;
  const long SV = c.S / V;
  const long units = (long)c.B * SV;   // V consecutive cells of one frame each
  const bool narrow = units <= 0x7fffffffL;
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;

  unsigned np[F][NT], tp[F][NT], nt[NT];   // per lane < 2^32 cells: the host caps B * S at 2^40
  double se[F], sa[F];
#pragma unroll
  for (int k = 0; k < NT; ++k) nt[k] = 0;
#pragma unroll
  for (int f = 0; f < F; ++f) {
    se[f] = sa[f] = 0.0;
#pragma unroll
    for (int k = 0; k < NT; ++k) np[f][k] = tp[f][k] = 0;
  }

  const float* tlead = c.tgt + (long)p * c.tl;
  const float* flead[F];
#pragma unroll
  for (int f = 0; f < F; ++f) flead[f] = c.field[f] + (long)p * c.fl[f];

  for (long u = (long)chunk * kBlock + threadIdx.x; u < units; u += (long)c.nchunk * kBlock) {
    long b, s;
    if (narrow) {
      const unsigned ub = (unsigned)u / (unsigned)SV;
      b = ub;
      s = (unsigned)u - ub * (unsigned)SV;
    } else {
      b = u / SV;
      s = u - b * SV;
    }
    s *= V;
    float t[V], v[F][V];
    load_cells<V>(tlead + b * c.tb + s, t);
#pragma unroll
    for (int f = 0; f < F; ++f) load_cells<V>(flead[f] + b * c.fb[f] + s, v[f]);
#pragma unroll
    for (int i = 0; i < V; ++i) {
      const float tv = c.clamp ? clamp01f(t[i]) : t[i];
      bool te[NT];
#pragma unroll
      for (int k = 0; k < NT; ++k) {
        te[k] = tv >= c.thr[k];
        nt[k] += te[k];
      }
#pragma unroll
      for (int f = 0; f < F; ++f) {
        const float fv = c.clamp ? clamp01f(v[f][i]) : v[f][i];
#pragma unroll
        for (int k = 0; k < NT; ++k) {
          const bool fe = fv >= c.thr[k];
          np[f][k] += fe;
          tp[f][k] += fe && te[k];
        }
        const double e = (double)fv - (double)tv;
        se[f] += e * e;
        sa[f] += fabs(e);
      }
    }
  }

#pragma unroll
  for (int k = 0; k < NT; ++k) {
    if (k < c.n_thr) {   // block-uniform
      const unsigned wt = wave_sum_u32(nt[k]);
#pragma unroll
      for (int f = 0; f < F; ++f) {
        const unsigned wp = wave_sum_u32(np[f][k]), wh = wave_sum_u32(tp[f][k]);
        if (lane == 0) {
          cnt_sm[wv][(f * kMaxThr + k) * 3] = wh;
          cnt_sm[wv][(f * kMaxThr + k) * 3 + 1] = wt - wh;
          cnt_sm[wv][(f * kMaxThr + k) * 3 + 2] = wp - wh;
        }
      }
    }
  }
  const long nblk = gridDim.x;
  const int ncnt = 3 * c.n_thr;
  double tot[2 * F];
#pragma unroll
  for (int f = 0; f < F; ++f) {
    tot[2 * f] = block_sum(se[f], sm);   // its barriers also publish cnt_sm
    tot[2 * f + 1] = block_sum(sa[f], sm);
  }
  if ((int)threadIdx.x < F * ncnt) {
    const int f = threadIdx.x / ncnt, j = threadIdx.x - f * ncnt;
    unsigned long long s = 0;
    for (int w = 0; w < kBlock / 64; ++w) s += cnt_sm[w][(f * kMaxThr + j / 3) * 3 + j % 3];
    rows[(long)threadIdx.x * nblk + blockIdx.x] = s;
  }
  if (threadIdx.x == 0) {
#pragma unroll
    for (int j = 0; j < 2 * F; ++j) rows[(long)(F * ncnt + j) * nblk + blockIdx.x] = __double_as_longlong(tot[j]);
  }
}

// one block per (lead, field), one thread per chunk: counts[lead][field] = [tp, fn, fp] x n_thr, cells;
// sums[lead][field] = sum e^2, sum |e|, the fp64 partials added in ascending chunk order
__global__ __launch_bounds__(kMaxChunks) void verify_finalize_kernel(const unsigned long long* __restrict__ rows, VerifyCfg c,
                                                                     int accumulate, long long* __restrict__ counts,
                                                                     double* __restrict__ sums) {
  __shared__ unsigned long long red[kMaxChunks / 64][3 * kMaxThr];
  __shared__ double part[2][kMaxChunks];
  const int p = blockIdx.x / c.F, f = blockIdx.x - p * c.F;
  const int ncnt = 3 * c.n_thr;
  const long nblk = (long)c.nchunk * c.P;
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const bool has = (int)threadIdx.x < c.nchunk;
  const long row = (long)threadIdx.x * c.P + p;
#pragma unroll
  for (int j = 0; j < 3 * kMaxThr; ++j) {
    unsigned long long v = (has && j < ncnt) ? rows[(long)(f * ncnt + j) * nblk + row] : 0ull;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    if (lane == 0) red[wv][j] = v;
  }
  part[0][threadIdx.x] = has ? __longlong_as_double(rows[(long)(c.F * ncnt + 2 * f) * nblk + row]) : 0.0;
  part[1][threadIdx.x] = has ? __longlong_as_double(rows[(long)(c.F * ncnt + 2 * f + 1) * nblk + row]) : 0.0;
  __syncthreads();
  long long* crow = counts + (long)blockIdx.x * (ncnt + 1);
  if ((int)threadIdx.x < ncnt) {
    unsigned long long t = 0;
    for (int w = 0; w < kMaxChunks / 64; ++w) t += red[w][threadIdx.x];
    crow[threadIdx.x] = (accumulate ? crow[threadIdx.x] : 0) + (long long)t;
  }
  if ((int)threadIdx.x == ncnt) crow[ncnt] = (accumulate ? crow[ncnt] : 0) + (long long)c.B * c.S;
  if (threadIdx.x == 64 || threadIdx.x == 128) {   // one wave each, neither the one that writes the counts
    const int q = threadIdx.x == 64 ? 0 : 1;
    double t = 0.0;   // rows past nchunk hold +0.0, which changes no bit of a sum of non-negative terms
#pragma unroll 16
    for (int i = 0; i < kMaxChunks; ++i) t += part[q][i];   // the loads of 16 adds in flight, the adds in order
    double* d = sums + (long)blockIdx.x * 2 + q;
    *d = (accumulate ? *d : 0.0) + t;
  }
}

template <int V, int NT>
void launch_part(const VerifyCfg& c, int nblk, unsigned long long* rows, hipStream_t st) {
  switch (c.F) {
    case 1: hipLaunchKernelGGL((verify_part_kernel<V, 1, NT>), dim3(nblk), dim3(kBlock), 0, st, c, rows); break;
    case 2: hipLaunchKernelGGL((verify_part_kernel<V, 2, NT>), dim3(nblk), dim3(kBlock), 0, st, c, rows); break;
    case 3: hipLaunchKernelGGL((verify_part_kernel<V, 3, NT>), dim3(nblk), dim3(kBlock), 0, st, c, rows); break;
    default: hipLaunchKernelGGL((verify_part_kernel<V, 4, NT>), dim3(nblk), dim3(kBlock), 0, st, c, rows); break;
  }
}

}  // namespace

extern "C" {

int wfae_verify_leads(const float* const* fields, const int64_t* field_bstride, const int64_t* field_lstride,
                      const float* target, int64_t target_bstride, int64_t target_lstride, int F, int B, int P, int64_t S,
                      const float* thresholds, int n_thr, int clamp01, int accumulate, int64_t* counts, double* sums,
                      void* ws, size_t ws_bytes, wfae_stream_t stream) {
  WFAE_REQUIRE(fields && field_bstride && field_lstride && target && counts && sums && ws, WFAE_ERR_NULL_POINTER,
               "verify_leads: null pointer");
  WFAE_REQUIRE(F >= 1 && F <= kMaxF, WFAE_ERR_BAD_SHAPE, "verify_leads: F %d not in [1, %d]", F, kMaxF);
  WFAE_REQUIRE(n_thr >= 0 && n_thr <= kMaxThr && (n_thr == 0 || thresholds), WFAE_ERR_BAD_SHAPE,
               "verify_leads: n_thr %d not in [0, %d]", n_thr, kMaxThr);
  WFAE_REQUIRE(B >= 1 && P >= 1 && S >= 1, WFAE_ERR_BAD_SHAPE, "verify_leads: bad shape B %d, P %d, S %lld", B, P,
               (long long)S);
  WFAE_REQUIRE((long)B * P <= (1L << 40) / S, WFAE_ERR_BAD_SHAPE, "verify_leads: tensor too large");
  WFAE_REQUIRE(target_bstride >= 0 && target_lstride >= 0, WFAE_ERR_BAD_SHAPE, "verify_leads: negative target stride");
  VerifyCfg c{};
  bool vec = S % 4 == 0 && (uintptr_t)target % 16 == 0 && target_bstride % 4 == 0 && target_lstride % 4 == 0;
  for (int f = 0; f < F; ++f) {
    WFAE_REQUIRE(fields[f], WFAE_ERR_NULL_POINTER, "verify_leads: null pointer (field %d)", f);
    WFAE_REQUIRE(field_bstride[f] >= 0 && field_lstride[f] >= 0, WFAE_ERR_BAD_SHAPE,
                 "verify_leads: negative stride of field %d", f);
    c.field[f] = fields[f];
    c.fb[f] = field_bstride[f];
    c.fl[f] = field_lstride[f];
    vec = vec && (uintptr_t)fields[f] % 16 == 0 && field_bstride[f] % 4 == 0 && field_lstride[f] % 4 == 0;
  }
  c.tgt = target;
  c.tb = target_bstride;
  c.tl = target_lstride;
  c.S = S;
  c.F = F;
  c.B = B;
  c.P = P;
  c.n_thr = n_thr;
  c.clamp = clamp01;
  for (int k = 0; k < kMaxThr; ++k) c.thr[k] = k < n_thr ? thresholds[k] : INFINITY;
  const long cells = (long)B * S;
  const long want = (cells + kCellsPerChunkTrip - 1) / kCellsPerChunkTrip;
  c.nchunk = (int)(want < kMaxChunks ? want : kMaxChunks);
  const long nblk = (long)c.nchunk * P;
  WFAE_REQUIRE(nblk <= 0x7fffffffL / kMaxF, WFAE_ERR_BAD_SHAPE, "verify_leads: too many leads (%d)", P);
  const size_t need = (size_t)nblk * F * (3 * n_thr + 2) * sizeof(unsigned long long);
  WFAE_REQUIRE(ws_bytes >= need, WFAE_ERR_BAD_SHAPE, "verify_leads: workspace %zu < %zu", ws_bytes, need);
  hipStream_t st = (hipStream_t)stream;
  unsigned long long* rows = (unsigned long long*)ws;
  if (vec) {
    if (n_thr <= 6) launch_part<4, 6>(c, (int)nblk, rows, st);
    else launch_part<4, kMaxThr>(c, (int)nblk, rows, st);
  } else {
    if (n_thr <= 6) launch_part<1, 6>(c, (int)nblk, rows, st);
    else launch_part<1, kMaxThr>(c, (int)nblk, rows, st);
  }
  int rc = check_launch("verify_part");
  if (rc) return rc;
  hipLaunchKernelGGL(verify_finalize_kernel, dim3(P * F), dim3(kMaxChunks), 0, st, (const unsigned long long*)ws, c,
                     accumulate, (long long*)counts, sums);
  return check_launch("verify_finalize");
}

}  // extern "C"
