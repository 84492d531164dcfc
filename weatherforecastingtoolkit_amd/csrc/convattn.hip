// convattn.hip — what the conv + attention latent autoencoder (experiments/v1_experiments/_convattn.py; reference
// pretrained_ae_convattn_ae_sevir/train.py:58-161) needs beyond the library's other families:
//   * attention with separate query / key lengths up to 256 (144 tokens of a 12 x 12 plane; heads of 16),
//   * GroupNorm (+ exact GELU) in training form, forward and backward,
//   * a per-channel bias, and the closed form of a one-key cross-attention with dropout.
// The arithmetic is tiny (~85 MFLOP per layer at B = 8): every kernel is launch- and latency-bound, so they are plain VALU
// kernels with one workgroup per (sample, head) or (sample, group), the operands of that workgroup held in LDS.  Nothing is
// reduced with atomics: every sum has a fixed order, so results are bitwise repeatable.
#include "common.h"

using namespace wfae;

namespace {

constexpr int kAttnD = 16;                 // head size served
constexpr int kAttnMaxS = WFAE_ATTN_MAX_S;  // 256
constexpr int kRow = kAttnD + 4;           // LDS row, 16-byte aligned: a row read by all lanes is 4 broadcast ds_read_b128

__device__ __forceinline__ float dot16(const float (&a)[kAttnD], const float* __restrict__ row) {
  float s = 0.f;
#pragma unroll
  for (int d = 0; d < kAttnD / 4; ++d) {
    const float4 r = *reinterpret_cast<const float4*>(row + 4 * d);
    s = fmaf(a[4 * d], r.x, s);
    s = fmaf(a[4 * d + 1], r.y, s);
    s = fmaf(a[4 * d + 2], r.z, s);
    s = fmaf(a[4 * d + 3], r.w, s);
  }
  return s;
}

__device__ __forceinline__ void axpy16(float (&acc)[kAttnD], float a, const float* __restrict__ row) {
#pragma unroll
  for (int d = 0; d < kAttnD / 4; ++d) {
    const float4 r = *reinterpret_cast<const float4*>(row + 4 * d);
    acc[4 * d] = fmaf(a, r.x, acc[4 * d]);
    acc[4 * d + 1] = fmaf(a, r.y, acc[4 * d + 1]);
    acc[4 * d + 2] = fmaf(a, r.z, acc[4 * d + 2]);
    acc[4 * d + 3] = fmaf(a, r.w, acc[4 * d + 3]);
  }
}

// rows [0, S) of head h of sample n, `stride` floats apart, into an LDS image of kRow-float rows
__device__ __forceinline__ void stage_rows(float (*dst)[kRow], const float* __restrict__ src, int S, long stride) {
  for (int e = threadIdx.x; e < S * kAttnD; e += blockDim.x) {
    const int r = e / kAttnD, d = e % kAttnD;
    dst[r][d] = src[(long)r * stride + d];
  }
}

// One workgroup per (n, h); thread i < Sq owns query row i.  K and V of the head sit in LDS (40 KiB at 256 keys).  The
// probability row in global memory is the thread's scratch for the scores, as in mha_fwd_kernel.
__global__ __launch_bounds__(256) void attn_fwd_kernel(const float* __restrict__ q, const float* __restrict__ k,
                                                       const float* __restrict__ v, float* __restrict__ out,
                                                       float* __restrict__ probs, int Sq, int Skv, int H, long qs, long ks_,
                                                       long vs_, float scale, float p_drop, unsigned long long seed) {
  __shared__ __attribute__((aligned(16))) float ks[kAttnMaxS][kRow], vs[kAttnMaxS][kRow];
  const int n = blockIdx.x / H, h = blockIdx.x % H;
  const int E = H * kAttnD;
  stage_rows(ks, k + (long)n * Skv * ks_ + h * kAttnD, Skv, ks_);
  stage_rows(vs, v + (long)n * Skv * vs_ + h * kAttnD, Skv, vs_);
  __syncthreads();
  const int i = threadIdx.x;
  if (i >= Sq) return;
  float qr[kAttnD];
  const float* qp = q + ((long)n * Sq + i) * qs + h * kAttnD;
#pragma unroll
  for (int d = 0; d < kAttnD; ++d) qr[d] = qp[d] * scale;
  const unsigned long long row_id = ((unsigned long long)n * H + h) * Sq + i;
  float* pr = probs + row_id * Skv;
  float mx = -INFINITY;
  for (int j = 0; j < Skv; ++j) {
    const float s = dot16(qr, ks[j]);
    pr[j] = s;
    mx = fmaxf(mx, s);
  }
  // the row sum in fp64: its rounding error scales every probability of the row alike (a coherent error, unlike the
  // independent roundings of the terms), and a serial fp32 chain over 256 terms is the worst order for it
  double den = 0.0;
  for (int j = 0; j < Skv; ++j) {
    const float e = expf(pr[j] - mx);
    pr[j] = e;
    den += (double)e;
  }
  const float inv = (float)(1.0 / den);
  const float keep = 1.f / (1.f - p_drop);
  float o[kAttnD];
#pragma unroll
  for (int d = 0; d < kAttnD; ++d) o[d] = 0.f;
  for (int j = 0; j < Skv; ++j) {
    float pj = pr[j] * inv;
    pr[j] = pj;   // the probabilities before dropout are what backward reads
    if (p_drop > 0.f) pj = rng01(seed, row_id * Skv + j) >= p_drop ? pj * keep : 0.f;
    axpy16(o, pj, vs[j]);
  }
  float* op = out + ((long)n * Sq + i) * E + h * kAttnD;
#pragma unroll
  for (int d = 0; d < kAttnD; ++d) op[d] = o[d];
}

// Backward, one workgroup per (n, h), two phases over the same 40 KiB of LDS.
//   phase 1 (thread = query row i; K and V in LDS):  dP_ij = m_ij (dout_i . v_j),  c_i = sum_j P_ij dP_ij,
//            dS_ij = P_ij (dP_ij - c_i),  dq_i = scale sum_j dS_ij k_j;  c_i is left in LDS.
//   phase 2 (thread = key row j; Q and dout in LDS):  dP_ij and dS_ij are formed again from P (read along j: coalesced),
//            c_i and the regenerated mask — 16 FMAs, instead of an Sq x Skv matrix that LDS cannot hold at 256 x 256 —
//            dk_j = scale sum_i dS_ij q_i,  dv_j = sum_i m_ij P_ij dout_i.
// m_ij = keep / (1 - p) or 0.  The i and j loops run in index order: fixed summation order, no atomics.
__global__ __launch_bounds__(256) void attn_bwd_kernel(const float* __restrict__ q, const float* __restrict__ k,
                                                       const float* __restrict__ v, const float* __restrict__ probs,
                                                       const float* __restrict__ dout, float* __restrict__ dq,
                                                       float* __restrict__ dk, float* __restrict__ dv, int Sq, int Skv, int H,
                                                       long qs, long ks_, long vs_, float scale, float p_drop,
                                                       unsigned long long seed) {
  __shared__ __attribute__((aligned(16))) float a[kAttnMaxS][kRow], b[kAttnMaxS][kRow];
  __shared__ float crow[kAttnMaxS];
  const int n = blockIdx.x / H, h = blockIdx.x % H;
  const int E = H * kAttnD;
  const int t = threadIdx.x;
  const unsigned long long head_row = ((unsigned long long)n * H + h) * Sq;
  const float keep = 1.f / (1.f - p_drop);
  const float* qh = q + (long)n * Sq * qs + h * kAttnD;
  const float* kh = k + (long)n * Skv * ks_ + h * kAttnD;
  const float* vh = v + (long)n * Skv * vs_ + h * kAttnD;
  const float* doh = dout + (long)n * Sq * E + h * kAttnD;

  stage_rows(a, kh, Skv, ks_);
  stage_rows(b, vh, Skv, vs_);
  __syncthreads();
  if (t < Sq) {
    float dor[kAttnD];
#pragma unroll
    for (int d = 0; d < kAttnD; ++d) dor[d] = doh[(long)t * E + d];
    const float* pr = probs + (head_row + t) * Skv;
    double cd = 0.0;   // fp64: c_i is subtracted from every dP_ij of the row, so its error is coherent over the row
    for (int j = 0; j < Skv; ++j) {
      float dp = dot16(dor, b[j]);
      if (p_drop > 0.f) dp *= rng01(seed, (head_row + t) * Skv + j) >= p_drop ? keep : 0.f;
      cd += (double)pr[j] * (double)dp;
    }
    const float c = (float)cd;
    crow[t] = c;
    float acc[kAttnD];
#pragma unroll
    for (int d = 0; d < kAttnD; ++d) acc[d] = 0.f;
    for (int j = 0; j < Skv; ++j) {
      float dp = dot16(dor, b[j]);
      if (p_drop > 0.f) dp *= rng01(seed, (head_row + t) * Skv + j) >= p_drop ? keep : 0.f;
      axpy16(acc, pr[j] * (dp - c), a[j]);
    }
    float* o = dq + (long)n * Sq * qs + (long)t * qs + h * kAttnD;
#pragma unroll
    for (int d = 0; d < kAttnD; ++d) o[d] = acc[d] * scale;
  }
  __syncthreads();
  stage_rows(a, qh, Sq, qs);
  stage_rows(b, doh, Sq, E);
  __syncthreads();
  if (t < Skv) {
    float vr[kAttnD], gk[kAttnD], gv[kAttnD];
#pragma unroll
    for (int d = 0; d < kAttnD; ++d) { vr[d] = vh[(long)t * vs_ + d]; gk[d] = 0.f; gv[d] = 0.f; }
    for (int i = 0; i < Sq; ++i) {
      float m = 1.f;
      if (p_drop > 0.f) m = rng01(seed, (head_row + i) * Skv + t) >= p_drop ? keep : 0.f;
      const float p = probs[(head_row + i) * Skv + t];
      // dout_i . v_j with the operands in phase 1's order (v from LDS there, from registers here: the same products)
      const float dp = dot16(vr, b[i]) * m;
      axpy16(gk, p * (dp - crow[i]), a[i]);
      axpy16(gv, p * m, b[i]);
    }
    float* ok = dk + (long)n * Skv * ks_ + (long)t * ks_ + h * kAttnD;
    float* ov = dv + (long)n * Skv * vs_ + (long)t * vs_ + h * kAttnD;
#pragma unroll
    for (int d = 0; d < kAttnD; ++d) { ok[d] = gk[d] * scale; ov[d] = gv[d]; }
  }
}

// ---------------------------------------------------------------- GroupNorm (+ GELU), training form
// One workgroup per (n, g); the group (C / G channels x HW, at most WFAE_GN_MAX_GROUP floats) is held in LDS between the
// passes.  Statistics are two-pass (the mean first, then the squared distances from it), summed in fp64.
__global__ __launch_bounds__(256) void gn_act_fwd_kernel(const float* __restrict__ x, const float* __restrict__ bias,
                                                         const float* __restrict__ gamma, const float* __restrict__ beta,
                                                         float* __restrict__ y, float* __restrict__ mean,
                                                         float* __restrict__ rstd, int C, int HW, int G, float eps, int act) {
  extern __shared__ float gn_lds[];
  __shared__ double red[16];
  __shared__ double bc;
  const int n = blockIdx.x / G, g = blockIdx.x % G;
  const int cpg = C / G, M = cpg * HW;
  const long base = ((long)n * C + (long)g * cpg) * HW;
  double s = 0.0;
  for (int e = threadIdx.x; e < M; e += 256) {
    float xv = x[base + e];
    if (bias) xv += bias[g * cpg + e / HW];
    gn_lds[e] = xv;
    s += (double)xv;
  }
  const float mu = (float)(block_sum_all(s, red, &bc) / (double)M);
  double ss = 0.0;
  for (int e = threadIdx.x; e < M; e += 256) {
    const float d = gn_lds[e] - mu;
    ss += (double)d * (double)d;
  }
  const float rs = (float)(1.0 / sqrt(block_sum_all(ss, red, &bc) / (double)M + (double)eps));
  for (int e = threadIdx.x; e < M; e += 256) {
    const int c = g * cpg + e / HW;
    const float z = (gn_lds[e] - mu) * rs * gamma[c] + beta[c];
    y[base + e] = act ? gelu_f(z) : z;
  }
  if (threadIdx.x == 0) { mean[blockIdx.x] = mu; rstd[blockIdx.x] = rs; }
}

// dz = dy act'(z) and xh are rebuilt from x and the two statistics and kept in LDS; a wave per channel forms
// sum_p dz xh and sum_p dz (fp64), which are this sample's share of dgamma / dbeta (part[(n C + c) 3 + {0, 1}]) and, weighted
// by gamma, the two group sums of  dx = rstd (gamma dz - mean(gamma dz) - xh mean(gamma dz xh)).  With a pre-bias its
// gradient is sum_p dx per channel (part[.. + 2]).
__global__ __launch_bounds__(256) void gn_act_bwd_kernel(const float* __restrict__ dy, const float* __restrict__ x,
                                                         const float* __restrict__ bias, const float* __restrict__ gamma,
                                                         const float* __restrict__ beta, const float* __restrict__ mean,
                                                         const float* __restrict__ rstd, float* __restrict__ dx,
                                                         float* __restrict__ part, int C, int HW, int G, int act) {
  extern __shared__ float gn_lds[];
  __shared__ double ws1[4], ws2[4];
  const int n = blockIdx.x / G, g = blockIdx.x % G;
  const int cpg = C / G, M = cpg * HW;
  float* xh = gn_lds;
  float* dz = gn_lds + M;
  const long base = ((long)n * C + (long)g * cpg) * HW;
  const float mu = mean[blockIdx.x], rs = rstd[blockIdx.x];
  for (int e = threadIdx.x; e < M; e += 256) {
    const int c = g * cpg + e / HW;
    float xv = x[base + e];
    if (bias) xv += bias[c];
    const float hh = (xv - mu) * rs;
    float d = dy[base + e];
    if (act) d *= gelu_grad_f(hh * gamma[c] + beta[c]);
    xh[e] = hh;
    dz[e] = d;
  }
  __syncthreads();
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  double s1 = 0.0, s2 = 0.0;   // sum_c gamma_c sum_p dz, sum_c gamma_c sum_p dz xh: this wave's channels
  for (int cl = wave; cl < cpg; cl += 4) {
    double sa = 0.0, sb = 0.0;
    for (int p = lane; p < HW; p += 64) {
      const float d = dz[cl * HW + p];
      sa += (double)d * (double)xh[cl * HW + p];
      sb += (double)d;
    }
    sa = wave_sum(sa);
    sb = wave_sum(sb);
    const int c = g * cpg + cl;
    if (lane == 0) {
      part[((long)n * C + c) * 3] = (float)sa;
      part[((long)n * C + c) * 3 + 1] = (float)sb;
    }
    s1 += (double)gamma[c] * sb;
    s2 += (double)gamma[c] * sa;
  }
  if (lane == 0) { ws1[wave] = s1; ws2[wave] = s2; }
  __syncthreads();
  // rounded once, like the product gamma dz below: a group of one element then cancels exactly (its dx is 0)
  const float m1 = (float)((ws1[0] + ws1[1] + ws1[2] + ws1[3]) / (double)M);
  const float m2 = (float)((ws2[0] + ws2[1] + ws2[2] + ws2[3]) / (double)M);
  for (int e = threadIdx.x; e < M; e += 256) {
    const int c = g * cpg + e / HW;
    const float gd = __fmul_rn(gamma[c], dz[e]);
    const float r = rs * ((gd - m1) - xh[e] * m2);
    dx[base + e] = r;
    if (bias) dz[e] = r;   // this thread's own element: no barrier needed before the store
  }
  if (!bias) return;
  __syncthreads();
  for (int cl = wave; cl < cpg; cl += 4) {
    double sa = 0.0;
    for (int p = lane; p < HW; p += 64) sa += (double)dz[cl * HW + p];
    sa = wave_sum(sa);
    if (lane == 0) part[((long)n * C + g * cpg + cl) * 3 + 2] = (float)sa;
  }
}

// dgamma / dbeta / dbias[c] (+)= sum_n part[(n C + c) 3 + k], n in order
__global__ __launch_bounds__(256) void gn_param_reduce_kernel(const float* __restrict__ part, int N, int C,
                                                              float* __restrict__ dgamma, float* __restrict__ dbeta,
                                                              float* __restrict__ dbias, int accumulate) {
  const int c = blockIdx.x * 256 + threadIdx.x;
  if (c >= C) return;
  double a = 0.0, b = 0.0, d = 0.0;
  for (int n = 0; n < N; ++n) {
    const float* p = part + ((long)n * C + c) * 3;
    a += (double)p[0];
    b += (double)p[1];
    if (dbias) d += (double)p[2];
  }
  dgamma[c] = (accumulate ? dgamma[c] : 0.f) + (float)a;
  dbeta[c] = (accumulate ? dbeta[c] : 0.f) + (float)b;
  if (dbias) dbias[c] = (accumulate ? dbias[c] : 0.f) + (float)d;
}

// ---------------------------------------------------------------- per-channel bias, one-key cross-attention
__global__ __launch_bounds__(256) void channel_bias_kernel(const float* __restrict__ x, const float* __restrict__ b,
                                                           float* __restrict__ y, long total, int C, int HW) {
  const long stride = (long)gridDim.x * blockDim.x;
  for (long e = (long)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += stride) y[e] = x[e] + b[(e / HW) % C];
}

// out[n][i][e] = v[n][e] m(n, e / D, i): with one key the softmax is 1, so attention is the value row under the mask
__global__ __launch_bounds__(256) void head_dropout_bcast_fwd_kernel(const float* __restrict__ v, float* __restrict__ out,
                                                                     long total, int Sq, int H, int D, float p_drop,
                                                                     unsigned long long seed) {
  const long stride = (long)gridDim.x * blockDim.x;
  const int E = H * D;
  const float keep = 1.f / (1.f - p_drop);
  for (long t = (long)blockIdx.x * blockDim.x + threadIdx.x; t < total; t += stride) {
    const int e = (int)(t % E);
    const long ni = t / E;
    const int i = (int)(ni % Sq);
    const long n = ni / Sq;
    float val = v[n * E + e];
    if (p_drop > 0.f) val = rng01(seed, ((unsigned long long)n * H + e / D) * Sq + i) >= p_drop ? val * keep : 0.f;
    out[t] = val;
  }
}

// dv[n][e] = sum_i dout[n][i][e] m(n, e / D, i), i in order; one thread per (n, e): the reads are coalesced along e
__global__ __launch_bounds__(256) void head_dropout_bcast_bwd_kernel(const float* __restrict__ dout, float* __restrict__ dv,
                                                                     long NE, int Sq, int H, int D, float p_drop,
                                                                     unsigned long long seed) {
  const long t = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= NE) return;
  const int E = H * D;
  const int e = (int)(t % E);
  const long n = t / E;
  const float keep = 1.f / (1.f - p_drop);
  const unsigned long long row0 = ((unsigned long long)n * H + e / D) * Sq;
  double s = 0.0;   // a plain sum of up to 256 terms that largely cancel: fp64, like the library's other column sums
  for (int i = 0; i < Sq; ++i) {
    float d = dout[(n * Sq + i) * E + e];
    if (p_drop > 0.f) d = rng01(seed, row0 + i) >= p_drop ? d * keep : 0.f;
    s += (double)d;
  }
  dv[t] = (float)s;
}

int attn_check(const char* what, int N, int Sq, int Skv, int H, int D, int64_t qs, int64_t ks, int64_t vs, float p_drop) {
  WFAE_REQUIRE(N > 0 && H > 0 && Sq > 0 && Skv > 0, WFAE_ERR_BAD_SHAPE, "%s: N, H, Sq, Skv must be positive", what);
  WFAE_REQUIRE(Sq <= kAttnMaxS && Skv <= kAttnMaxS, WFAE_ERR_BAD_SHAPE, "%s: Sq = %d, Skv = %d, served up to %d", what, Sq,
               Skv, kAttnMaxS);
  if (D != kAttnD) return fail(WFAE_ERR_UNSUPPORTED, "%s: head dim %d (16 built)", what, D);
  const int64_t E = (int64_t)H * D;
  WFAE_REQUIRE(qs >= E && ks >= E && vs >= E, WFAE_ERR_BAD_SHAPE, "%s: a row stride is shorter than H * D = %lld", what,
               (long long)E);
  WFAE_REQUIRE((int64_t)N * H <= 0x7fffffff, WFAE_ERR_BAD_SHAPE, "%s: N * H exceeds one grid dimension", what);
  WFAE_REQUIRE(p_drop >= 0.f && p_drop < 1.f, WFAE_ERR_BAD_SHAPE, "%s: dropout probability", what);
  return WFAE_OK;
}

inline int attn_threads(int Sq, int Skv) {
  const int s = Sq > Skv ? Sq : Skv;
  return ((s + 63) / 64) * 64;
}

}  // namespace

extern "C" {

int wfae_attn_fwd(const float* q, const float* k, const float* v, float* out, float* probs, int N, int Sq, int Skv, int H,
                  int D, int64_t q_stride, int64_t k_stride, int64_t v_stride, float p_drop, uint64_t seed,
                  wfae_stream_t stream) {
  WFAE_REQUIRE(q && k && v && out && probs, WFAE_ERR_NULL_POINTER, "attn_fwd: null pointer");
  const int rc = attn_check("attn_fwd", N, Sq, Skv, H, D, q_stride, k_stride, v_stride, p_drop);
  if (rc) return rc;
  hipLaunchKernelGGL(attn_fwd_kernel, dim3(N * H), dim3(attn_threads(Sq, Skv)), 0, (hipStream_t)stream, q, k, v, out, probs,
                     Sq, Skv, H, (long)q_stride, (long)k_stride, (long)v_stride, 1.0f / sqrtf((float)D), p_drop,
                     (unsigned long long)seed);
  return check_launch("attn_fwd");
}

int wfae_attn_bwd(const float* q, const float* k, const float* v, const float* probs, const float* dout, float* dq, float* dk,
                  float* dv, int N, int Sq, int Skv, int H, int D, int64_t q_stride, int64_t k_stride, int64_t v_stride,
                  float p_drop, uint64_t seed, wfae_stream_t stream) {
  WFAE_REQUIRE(q && k && v && probs && dout && dq && dk && dv, WFAE_ERR_NULL_POINTER, "attn_bwd: null pointer");
  const int rc = attn_check("attn_bwd", N, Sq, Skv, H, D, q_stride, k_stride, v_stride, p_drop);
  if (rc) return rc;
  hipLaunchKernelGGL(attn_bwd_kernel, dim3(N * H), dim3(attn_threads(Sq, Skv)), 0, (hipStream_t)stream, q, k, v, probs, dout,
                     dq, dk, dv, Sq, Skv, H, (long)q_stride, (long)k_stride, (long)v_stride, 1.0f / sqrtf((float)D), p_drop,
                     (unsigned long long)seed);
  return check_launch("attn_bwd");
}

size_t wfae_gn_act_bwd_workspace_bytes(int N, int C) {
  if (N < 1 || C < 1) return 0;
  return (size_t)N * (size_t)C * 3 * sizeof(float);
}

// A launch may ask for more than 64 KiB of LDS only after the kernel has been told so.  The kernels' own static LDS (below
// 1 KiB) counts against the same default, so the line is drawn at 63 KiB of dynamic LDS; the workload's groups (18 KiB
// forward, 36 KiB backward) stay below it and pay no runtime call.  The attribute is set to the kernel's largest request,
// `most`, whatever this launch needs, so that concurrent callers cannot lower it under one another.
static int gn_allow_lds(const char* what, const void* kernel, size_t lds, size_t most) {
  if (lds <= 63 * 1024) return WFAE_OK;
  const hipError_t e = hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)most);
  if (e != hipSuccess)
    return fail(WFAE_ERR_LAUNCH, "%s: %zu bytes of dynamic LDS were not granted: %s", what, lds, hipGetErrorString(e));
  return WFAE_OK;
}

static int gn_check(const char* what, int N, int C, int HW, int G, int act) {
  WFAE_REQUIRE(N > 0 && C > 0 && HW > 0 && G > 0, WFAE_ERR_BAD_SHAPE, "%s: N, C, HW, G must be positive", what);
  WFAE_REQUIRE(C % G == 0, WFAE_ERR_BAD_SHAPE, "%s: %d channels are not divisible by %d groups", what, C, G);
  WFAE_REQUIRE(act == 0 || act == 1, WFAE_ERR_BAD_SHAPE, "%s: act %d (0 = none, 1 = GELU)", what, act);
  WFAE_REQUIRE((int64_t)N * G <= 0x7fffffff && (int64_t)N * C * HW <= 0x7fffffff, WFAE_ERR_BAD_SHAPE, "%s: tensor too large",
               what);
  if ((int64_t)(C / G) * HW > WFAE_GN_MAX_GROUP)
    return fail(WFAE_ERR_UNSUPPORTED, "%s: a group of %d x %d = %lld elements, the on-chip form serves <= %d", what, C / G, HW,
                (long long)(C / G) * HW, WFAE_GN_MAX_GROUP);
  return WFAE_OK;
}

int wfae_gn_act_fwd(const float* x, const float* bias, const float* gamma, const float* beta, float* y, float* mean,
                    float* rstd, int N, int C, int HW, int G, float eps, int act, wfae_stream_t stream) {
  WFAE_REQUIRE(x && gamma && beta && y && mean && rstd, WFAE_ERR_NULL_POINTER, "gn_act_fwd: null pointer");
  const int rc = gn_check("gn_act_fwd", N, C, HW, G, act);
  if (rc) return rc;
  WFAE_REQUIRE(eps >= 0.f, WFAE_ERR_BAD_SHAPE, "gn_act_fwd: eps");
  const size_t lds = (size_t)(C / G) * HW * sizeof(float);
  const int rl = gn_allow_lds("gn_act_fwd", (const void*)gn_act_fwd_kernel, lds, WFAE_GN_MAX_GROUP * sizeof(float));
  if (rl) return rl;
  hipLaunchKernelGGL(gn_act_fwd_kernel, dim3(N * G), dim3(256), lds, (hipStream_t)stream, x, bias, gamma, beta, y, mean, rstd,
                     C, HW, G, eps, act);
  return check_launch("gn_act_fwd");
}

int wfae_gn_act_bwd(const float* dy, const float* x, const float* bias, const float* gamma, const float* beta,
                    const float* mean, const float* rstd, float* dx, float* dgamma, float* dbeta, float* dbias, int N, int C,
                    int HW, int G, int act, int accumulate, void* ws, size_t ws_bytes, wfae_stream_t stream) {
  WFAE_REQUIRE(dy && x && gamma && beta && mean && rstd && dx && dgamma && dbeta, WFAE_ERR_NULL_POINTER,
               "gn_act_bwd: null pointer");
  WFAE_REQUIRE((bias == nullptr) == (dbias == nullptr), WFAE_ERR_NULL_POINTER,
               "gn_act_bwd: bias and dbias are given together or not at all");
  const int rc = gn_check("gn_act_bwd", N, C, HW, G, act);
  if (rc) return rc;
  WFAE_REQUIRE(ws && ws_bytes >= wfae_gn_act_bwd_workspace_bytes(N, C), WFAE_ERR_WORKSPACE, "gn_act_bwd: workspace");
  hipStream_t st = (hipStream_t)stream;
  const size_t lds = (size_t)2 * (C / G) * HW * sizeof(float);
  const int rl = gn_allow_lds("gn_act_bwd", (const void*)gn_act_bwd_kernel, lds, 2 * WFAE_GN_MAX_GROUP * sizeof(float));
  if (rl) return rl;
  hipLaunchKernelGGL(gn_act_bwd_kernel, dim3(N * G), dim3(256), lds, st, dy, x, bias, gamma, beta, mean, rstd, dx, (float*)ws,
                     C, HW, G, act);
  int rc2 = check_launch("gn_act_bwd");
  if (rc2) return rc2;
  hipLaunchKernelGGL(gn_param_reduce_kernel, dim3(cdiv(C, 256)), dim3(256), 0, st, (const float*)ws, N, C, dgamma, dbeta,
                     dbias, accumulate);
  return check_launch("gn_act_bwd_reduce");
}

int wfae_channel_bias_fwd(const float* x, const float* b, float* y, int N, int C, int HW, wfae_stream_t stream) {
  WFAE_REQUIRE(x && b && y, WFAE_ERR_NULL_POINTER, "channel_bias_fwd: null pointer");
  WFAE_REQUIRE(N > 0 && C > 0 && HW > 0, WFAE_ERR_BAD_SHAPE, "channel_bias_fwd: N, C, HW must be positive");
  const long total = (long)N * C * HW;
  hipLaunchKernelGGL(channel_bias_kernel, dim3(grid_1d(total)), dim3(256), 0, (hipStream_t)stream, x, b, y, total, C, HW);
  return check_launch("channel_bias_fwd");
}

static int hdb_check(const char* what, int N, int Sq, int H, int D, float p_drop) {
  WFAE_REQUIRE(N > 0 && Sq > 0 && H > 0 && D > 0, WFAE_ERR_BAD_SHAPE, "%s: N, Sq, H, D must be positive", what);
  WFAE_REQUIRE((int64_t)H * D <= 0x7fffffff, WFAE_ERR_BAD_SHAPE, "%s: H * D too large", what);
  WFAE_REQUIRE(p_drop >= 0.f && p_drop < 1.f, WFAE_ERR_BAD_SHAPE, "%s: dropout probability", what);
  return WFAE_OK;
}

int wfae_head_dropout_bcast_fwd(const float* v, float* out, int N, int Sq, int H, int D, float p_drop, uint64_t seed,
                                wfae_stream_t stream) {
  WFAE_REQUIRE(v && out, WFAE_ERR_NULL_POINTER, "head_dropout_bcast_fwd: null pointer");
  const int rc = hdb_check("head_dropout_bcast_fwd", N, Sq, H, D, p_drop);
  if (rc) return rc;
  const long total = (long)N * Sq * H * D;
  hipLaunchKernelGGL(head_dropout_bcast_fwd_kernel, dim3(grid_1d(total)), dim3(256), 0, (hipStream_t)stream, v, out, total, Sq,
                     H, D, p_drop, (unsigned long long)seed);
  return check_launch("head_dropout_bcast_fwd");
}

int wfae_head_dropout_bcast_bwd(const float* dout, float* dv, int N, int Sq, int H, int D, float p_drop, uint64_t seed,
                                wfae_stream_t stream) {
  WFAE_REQUIRE(dout && dv, WFAE_ERR_NULL_POINTER, "head_dropout_bcast_bwd: null pointer");
  const int rc = hdb_check("head_dropout_bcast_bwd", N, Sq, H, D, p_drop);
  if (rc) return rc;
  const long NE = (long)N * H * D;
  hipLaunchKernelGGL(head_dropout_bcast_bwd_kernel, dim3(cdiv(NE, 256)), dim3(256), 0, (hipStream_t)stream, dout, dv, NE, Sq, H,
                     D, p_drop, (unsigned long long)seed);
  return check_launch("head_dropout_bcast_bwd");
}

}  // extern "C"
