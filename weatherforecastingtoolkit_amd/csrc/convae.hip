// convae.hip — kernels of the conv latent autoencoder (reference experiments/v1_experiments/pretrained_ae_convae_sevir/
// train.py:58-143 `ConvEncoder`, `ConvDecoder`, `ConvModel`); its Huber loss is in loss.hip.
//
// The fused unit ("CLN"):  y = LeakyReLU_slope(LayerNorm_sample(conv(x) + bias) * gamma + beta)  for the three convolution
// kinds of the model, all with padding 1:  kind 0 = Conv2d 3x3 stride 1, kind 1 = Conv2d 4x4 stride 2,
// kind 2 = ConvTranspose2d 4x4 stride 2 (weight (Cin, Cout, 4, 4)).  LayerNorm is nn.LayerNorm([C, H, W]): one mean and
// one biased variance per SAMPLE over all E = Cout Ho Wo elements, gamma / beta per element.
//
// One workgroup of 1024 threads owns one sample.  Forward: the weights, the sample's input x (when it fits) and then the
// whole pre-norm output u of the sample live in LDS (E <= 18432 floats = 72 KiB, weights <= 64 KiB); mean and variance are
// taken over u in two passes (per-thread fp32 partials in a fixed element order, block reduction in fp64), and y, x_hat,
// mean, rstd are written — u never reaches memory.  Backward: the activation mask is recomputed from a = gamma x_hat + beta, the LayerNorm data gradient du of the
// sample is formed in LDS, and the same workgroup takes the convolution's data gradient and the sample's weight / bias
// gradient partials from it; a finalize kernel sums the partials (and dgamma / dbeta) over the samples in ascending order.
// Where x does not fit LDS next to u (Cin = 64 at 24 x 24) it is read from global memory (it stays in L2); the tap loops
// reading it from there are latency-bound, which is why it is staged whenever it fits.
// No atomics: two launches on the same inputs give the same bits.
#include "common.h"

using namespace wfae;

namespace {

constexpr int kThreads = 1024;
constexpr int kCoutMax = 16;
constexpr int kCinMax = 64;
constexpr int kEMax = 18432;         // 8 x 48 x 48: the widest activation of the reference model
constexpr size_t kLdsLimit = 160 * 1024;
constexpr float kLnEps = 1e-5f;      // nn.LayerNorm default

struct ClnShape {
  int N, Cin, Cout, H, W, Ho, Wo;    // x (N, Cin, H, W) -> y (N, Cout, Ho, Wo)
  float slope;
};

// One axis of the tap geometry (padding 1).  DIRECT: the source index of destination d under tap k is d S - 1 + k (a
// convolution read from its output side, a transposed one from its input side).  Otherwise d = s S - 1 + k has to hold
// for an integer s: the scattering direction turned into a gather.
template <int S, bool DIRECT>
__device__ __forceinline__ bool tap_src(int d, int k, int lim, int& s) {
  if (DIRECT) {
    s = d * S - 1 + k;
    return s >= 0 && s < lim;
  }
  const int t = d + 1 - k;
  if (t < 0 || (t % S) != 0) return false;
  s = t / S;
  return s < lim;
}

template <bool T>
__device__ __forceinline__ int w_index(int co, int ci, int tap, int Cin, int Cout, int KK) {
  return T ? (ci * Cout + co) * KK + tap : (co * Cin + ci) * KK + tap;
}

// LDS layout of both kernels: [16 + 2 doubles][u / du: E floats, padded to 4][weights, transposed to [tap][ci][co padded
// to 4]: one 16-byte read gives four output channels][XL: the sample's input x][backward: weight-gradient slice partials]
__host__ __device__ inline int pad4(int v) { return (v + 3) & ~3; }

// stage the weights as Wl[(tap * Cin + ci) * CP + co] (zero in the padding)
template <bool T>
__device__ __forceinline__ void stage_weights(const float* __restrict__ w, float* Wl, int Cin, int Cout, int KK, int CP) {
  const int n = KK * Cin * CP;
  for (int i = threadIdx.x; i < n; i += kThreads) {
    const int co = i % CP, r = i / CP, ci = r % Cin, tap = r / Cin;
    Wl[i] = co < Cout ? w[w_index<T>(co, ci, tap, Cin, Cout, KK)] : 0.f;
  }
}

template <int K, int S, bool T, bool XL>
__global__ __launch_bounds__(kThreads) void wfae_cln_fwd_kernel(const float* __restrict__ x, const float* __restrict__ w,
                                                                const float* __restrict__ bias,
                                                                const float* __restrict__ gamma,
                                                                const float* __restrict__ beta, float* __restrict__ y,
                                                                float* __restrict__ xhat, float* __restrict__ mean,
                                                                float* __restrict__ rstd, ClnShape s) {
  extern __shared__ double smd[];
  constexpr int KK = K * K;
  double* red = smd;
  double* bc = smd + 16;
  float* U = reinterpret_cast<float*>(smd + 18);
  const int HWo = s.Ho * s.Wo, HWi = s.H * s.W, E = s.Cout * HWo, CP = pad4(s.Cout);
  float* Wl = U + pad4(E);
  float* Xl = Wl + KK * s.Cin * CP;
  const int n = blockIdx.x;
  const float* __restrict__ xs = x + (long)n * s.Cin * HWi;
  stage_weights<T>(w, Wl, s.Cin, s.Cout, KK, CP);
  if (XL)
    for (int i = threadIdx.x; i < s.Cin * HWi; i += kThreads) Xl[i] = xs[i];
  __syncthreads();
  const float* xin = XL ? Xl : xs;

  // convolution + bias: one thread per output pixel, all output channels in registers
  for (int p = threadIdx.x; p < HWo; p += kThreads) {
    const int oy = p / s.Wo, ox = p % s.Wo;
    float acc[kCoutMax];
#pragma unroll
    for (int co = 0; co < kCoutMax; ++co) acc[co] = co < s.Cout ? bias[co] : 0.f;
    for (int ky = 0; ky < K; ++ky) {
      int iy;
      if (!tap_src<S, !T>(oy, ky, s.H, iy)) continue;
      float row[kCoutMax];   // one kernel row on its own, then added: shorter rounding chains at Cin = 64
#pragma unroll
      for (int co = 0; co < kCoutMax; ++co) row[co] = 0.f;
      for (int kx = 0; kx < K; ++kx) {
        int ix;
        if (!tap_src<S, !T>(ox, kx, s.W, ix)) continue;
        const float* xp = xin + iy * s.W + ix;
        const float* wp = Wl + (ky * K + kx) * s.Cin * CP;
        for (int ci = 0; ci < s.Cin; ++ci) {
          const float v = xp[ci * HWi];
#pragma unroll
          for (int c4 = 0; c4 < kCoutMax / 4; ++c4)
            if (c4 * 4 < s.Cout) {
              const float4 wv = *reinterpret_cast<const float4*>(wp + ci * CP + c4 * 4);
              row[c4 * 4 + 0] = fmaf(v, wv.x, row[c4 * 4 + 0]);
              row[c4 * 4 + 1] = fmaf(v, wv.y, row[c4 * 4 + 1]);
              row[c4 * 4 + 2] = fmaf(v, wv.z, row[c4 * 4 + 2]);
              row[c4 * 4 + 3] = fmaf(v, wv.w, row[c4 * 4 + 3]);
            }
        }
      }
#pragma unroll
      for (int co = 0; co < kCoutMax; ++co) acc[co] += row[co];
    }
#pragma unroll
    for (int co = 0; co < kCoutMax; ++co)
      if (co < s.Cout) U[co * HWo + p] = acc[co];
  }
  __syncthreads();

  // two-pass statistics over the sample
  float part = 0.f;
  for (int e = threadIdx.x; e < E; e += kThreads) part += U[e];
  const float mu = (float)(block_sum_all((double)part, red, bc) / (double)E);
  part = 0.f;
  for (int e = threadIdx.x; e < E; e += kThreads) {
    const float d = U[e] - mu;
    part = fmaf(d, d, part);
  }
  const float var = (float)(block_sum_all((double)part, red, bc) / (double)E);
  const float rs = 1.0f / sqrtf(var + kLnEps);
  if (threadIdx.x == 0) {
    mean[n] = mu;
    rstd[n] = rs;
  }
  float* __restrict__ ys = y + (long)n * E;
  float* __restrict__ hs = xhat + (long)n * E;
  for (int e = threadIdx.x; e < E; e += kThreads) {
    const float h = (U[e] - mu) * rs;
    const float a = fmaf(gamma[e], h, beta[e]);
    hs[e] = h;
    ys[e] = a > 0.f ? a : s.slope * a;
  }
}

// per sample: du (LDS) from dy, x_hat, rstd, gamma, beta; dx (when asked for); the sample's weight / bias gradient partials
// dwp[n][nW], dbp[n][Cout]
template <int K, int S, bool T, bool XL>
__global__ __launch_bounds__(kThreads) void wfae_cln_bwd_sample_kernel(
    const float* __restrict__ dy, const float* __restrict__ xhat, const float* __restrict__ rstd,
    const float* __restrict__ gamma, const float* __restrict__ beta, const float* __restrict__ x,
    const float* __restrict__ w, float* __restrict__ dx, float* __restrict__ dwp, float* __restrict__ dbp, ClnShape s,
    int nslices) {
  extern __shared__ double smd[];
  constexpr int KK = K * K;
  double* red = smd;
  double* bc = smd + 16;
  float* DU = reinterpret_cast<float*>(smd + 18);
  const int HWo = s.Ho * s.Wo, HWi = s.H * s.W, E = s.Cout * HWo, nW = s.Cout * s.Cin * KK, CP = pad4(s.Cout);
  float* Wl = DU + pad4(E);                      // only when dx is asked for
  float* Xl = Wl + (dx ? KK * s.Cin * CP : 0);
  float* SL = Xl + (XL ? s.Cin * HWi : 0);       // nslices * nW floats, only when nslices > 1
  const int n = blockIdx.x;
  const float* __restrict__ gs = dy + (long)n * E;
  const float* __restrict__ hs = xhat + (long)n * E;
  const float* __restrict__ xs = x + (long)n * s.Cin * HWi;
  if (dx) stage_weights<T>(w, Wl, s.Cin, s.Cout, KK, CP);
  if (XL)
    for (int i = threadIdx.x; i < s.Cin * HWi; i += kThreads) Xl[i] = xs[i];
  const float* xin = XL ? Xl : xs;

  // activation mask + affine: DU <- dL/dx_hat, and its two sums over the sample
  float p1 = 0.f, p2 = 0.f;
  for (int e = threadIdx.x; e < E; e += kThreads) {
    const float h = hs[e], gm = gamma[e];
    const float a = fmaf(gm, h, beta[e]);
    const float g = gs[e] * (a > 0.f ? 1.0f : s.slope) * gm;
    DU[e] = g;
    p1 += g;
    p2 = fmaf(g, h, p2);
  }
  const float m1 = (float)(block_sum_all((double)p1, red, bc) / (double)E);
  const float m2 = (float)(block_sum_all((double)p2, red, bc) / (double)E);
  const float rs = rstd[n];
  for (int e = threadIdx.x; e < E; e += kThreads) DU[e] = rs * (DU[e] - m1 - hs[e] * m2);
  __syncthreads();

  // data gradient: one thread per input element
  if (dx) {
    float* __restrict__ dxs = dx + (long)n * s.Cin * HWi;
    for (int i = threadIdx.x; i < s.Cin * HWi; i += kThreads) {
      const int ci = i / HWi, q = i % HWi, iy = q / s.W, ix = q % s.W;
      float acc = 0.f;
      for (int ky = 0; ky < K; ++ky) {
        int oy;
        if (!tap_src<S, T>(iy, ky, s.Ho, oy)) continue;
        for (int kx = 0; kx < K; ++kx) {
          int ox;
          if (!tap_src<S, T>(ix, kx, s.Wo, ox)) continue;
          const float* d = DU + oy * s.Wo + ox;
          const float* wp = Wl + ((ky * K + kx) * s.Cin + ci) * CP;
#pragma unroll
          for (int c4 = 0; c4 < kCoutMax / 4; ++c4)
            if (c4 * 4 < s.Cout) {
              const float4 wv = *reinterpret_cast<const float4*>(wp + c4 * 4);
              const int c = c4 * 4;   // the padding of wv is zero; du is read inside the sample only
              acc = fmaf(d[c * HWo], wv.x, acc);
              if (c + 1 < s.Cout) acc = fmaf(d[(c + 1) * HWo], wv.y, acc);
              if (c + 2 < s.Cout) acc = fmaf(d[(c + 2) * HWo], wv.z, acc);
              if (c + 3 < s.Cout) acc = fmaf(d[(c + 3) * HWo], wv.w, acc);
            }
        }
      }
      dxs[i] = acc;
    }
  }

  // bias gradient partial: one wavefront per output channel
  {
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    for (int co = wv; co < s.Cout; co += kThreads / 64) {
      float a = 0.f;
      for (int p = lane; p < HWo; p += 64) a += DU[co * HWo + p];
      a = wave_sum(a);
      if (lane == 0) dbp[(long)n * s.Cout + co] = a;
    }
  }

  // weight gradient partial: thread (input channel, tap, output-row slice) with all output channels in registers, so x is
  // read once per pixel; per output row, then added (the sum over a 48 x 48 plane is not one 2304-term chain); slices
  // are summed in ascending order
  float* __restrict__ dws = dwp + (long)n * nW;
  const int items = s.Cin * KK;
  for (int i = threadIdx.x; i < items * nslices; i += kThreads) {
    const int j = i % items, sl = i / items;
    const int ci = j / KK, tap = j % KK, ky = tap / K, kx = tap % K;
    const float* xc = xin + ci * HWi;
    float acc[kCoutMax];
#pragma unroll
    for (int co = 0; co < kCoutMax; ++co) acc[co] = 0.f;
    for (int oy = sl; oy < s.Ho; oy += nslices) {
      int iy;
      if (!tap_src<S, !T>(oy, ky, s.H, iy)) continue;
      float row[kCoutMax];
#pragma unroll
      for (int co = 0; co < kCoutMax; ++co) row[co] = 0.f;
      for (int ox = 0; ox < s.Wo; ++ox) {
        int ix;
        if (!tap_src<S, !T>(ox, kx, s.W, ix)) continue;
        const float xv = xc[iy * s.W + ix];
        const float* d = DU + oy * s.Wo + ox;
#pragma unroll
        for (int co = 0; co < kCoutMax; ++co)
          if (co < s.Cout) row[co] = fmaf(d[co * HWo], xv, row[co]);
      }
#pragma unroll
      for (int co = 0; co < kCoutMax; ++co) acc[co] += row[co];
    }
#pragma unroll
    for (int co = 0; co < kCoutMax; ++co)
      if (co < s.Cout) {
        const int wi = w_index<T>(co, ci, tap, s.Cin, s.Cout, KK);
        if (nslices == 1) dws[wi] = acc[co];
        else SL[sl * nW + wi] = acc[co];
      }
  }
  if (nslices > 1) {
    __syncthreads();
    for (int wi = threadIdx.x; wi < nW; wi += kThreads) {
      float acc = 0.f;
      for (int sl = 0; sl < nslices; ++sl) acc += SL[sl * nW + wi];
      dws[wi] = acc;
    }
  }
}

// dgamma[e] = sum_n g x_hat, dbeta[e] = sum_n g (g = dy * mask, recomputed); dw, dbias = sums of the sample partials.
// All over n ascending.
__global__ __launch_bounds__(256) void wfae_cln_bwd_final_kernel(const float* __restrict__ dy,
                                                                 const float* __restrict__ xhat,
                                                                 const float* __restrict__ gamma,
                                                                 const float* __restrict__ beta,
                                                                 const float* __restrict__ dwp,
                                                                 const float* __restrict__ dbp, float* __restrict__ dgamma,
                                                                 float* __restrict__ dbeta, float* __restrict__ dw,
                                                                 float* __restrict__ dbias, int N, int E, int nW, int Cout,
                                                                 float slope) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < E) {
    const float gm = gamma[i], bt = beta[i];
    float a1 = 0.f, a2 = 0.f;
    for (int n = 0; n < N; ++n) {
      const float h = xhat[(long)n * E + i];
      const float g = dy[(long)n * E + i] * (fmaf(gm, h, bt) > 0.f ? 1.0f : slope);
      a1 = fmaf(g, h, a1);
      a2 += g;
    }
    dgamma[i] = a1;
    dbeta[i] = a2;
  } else if (i < E + nW) {
    const int j = i - E;
    float a = 0.f;
    for (int n = 0; n < N; ++n) a += dwp[(long)n * nW + j];
    dw[j] = a;
  } else if (i < E + nW + Cout) {
    const int j = i - E - nW;
    float a = 0.f;
    for (int n = 0; n < N; ++n) a += dbp[(long)n * Cout + j];
    dbias[j] = a;
  }
}

int cln_shape(const char* what, int kind, int N, int Cin, int Cout, int H, int W, float slope, ClnShape* s) {
  WFAE_REQUIRE(kind >= 0 && kind <= 2, WFAE_ERR_BAD_SHAPE,
               "%s: kind %d (0 = 3x3 s1, 1 = 4x4 s2, 2 = transposed 4x4 s2)", what, kind);
  WFAE_REQUIRE(N > 0 && N <= 65535 && Cin > 0 && Cout > 0 && H > 0 && W > 0, WFAE_ERR_BAD_SHAPE,
               "%s: bad shape N=%d Cin=%d Cout=%d H=%d W=%d", what, N, Cin, Cout, H, W);
  WFAE_REQUIRE(Cin <= kCinMax, WFAE_ERR_UNSUPPORTED, "%s: Cin = %d, the fused unit serves Cin <= %d", what, Cin, kCinMax);
  WFAE_REQUIRE(Cout <= kCoutMax, WFAE_ERR_UNSUPPORTED, "%s: Cout = %d, the fused unit serves Cout <= %d", what, Cout,
               kCoutMax);
  WFAE_REQUIRE(kind != 1 || (H % 2 == 0 && W % 2 == 0), WFAE_ERR_BAD_SHAPE,
               "%s: the 4x4 stride-2 convolution needs an even input plane (got %dx%d)", what, H, W);
  int Ho = H, Wo = W;
  if (kind == 1) Ho = H / 2, Wo = W / 2;
  if (kind == 2) {
    WFAE_REQUIRE(H <= 16384 && W <= 16384, WFAE_ERR_UNSUPPORTED, "%s: plane %dx%d too large", what, H, W);
    Ho = 2 * H, Wo = 2 * W;
  }
  const long E = (long)Cout * Ho * Wo;
  WFAE_REQUIRE(E <= kEMax, WFAE_ERR_UNSUPPORTED,
               "%s: output sample Cout*Ho*Wo = %ld elements, the fused unit serves <= %d (it is held in LDS)", what, E,
               kEMax);
  *s = ClnShape{N, Cin, Cout, H, W, Ho, Wo, slope};
  return 0;
}

inline int cln_kk(int kind) { return kind == 0 ? 9 : 16; }

// sample partials of the weight and bias gradients
inline size_t cln_ws_bytes(int kind, int N, int Cin, int Cout) {
  return (size_t)N * ((size_t)Cout * Cin * cln_kk(kind) + Cout) * sizeof(float);
}

}  // namespace

extern "C" {

int wfae_cln_fwd(const float* x, const float* w, const float* bias, const float* gamma, const float* beta, float* y,
                 float* xhat, float* mean, float* rstd, int kind, int N, int Cin, int Cout, int H, int W, float slope,
                 wfae_stream_t stream) {
  WFAE_REQUIRE(x && w && bias && gamma && beta && y && xhat && mean && rstd, WFAE_ERR_NULL_POINTER,
               "cln_fwd: null pointer");
  ClnShape s;
  int rc = cln_shape("cln_fwd", kind, N, Cin, Cout, H, W, slope, &s);
  if (rc) return rc;
  const size_t E4 = pad4(Cout * s.Ho * s.Wo), nWp = (size_t)cln_kk(kind) * Cin * pad4(Cout), nX = (size_t)Cin * H * W;
  size_t lds = 18 * sizeof(double) + (E4 + nWp + nX) * sizeof(float);
  const bool xl = lds <= kLdsLimit;   // the sample's input next to its output in LDS when both fit
  if (!xl) lds -= nX * sizeof(float);
  WFAE_REQUIRE(lds <= kLdsLimit, WFAE_ERR_UNSUPPORTED, "cln_fwd: %zu bytes of LDS > %zu", lds, kLdsLimit);
  hipStream_t st = (hipStream_t)stream;
#define WFAE_CLN_F(K_, S_, T_, XL_)                                                                               \
  do {                                                                                                            \
    (void)hipFuncSetAttribute((const void*)wfae_cln_fwd_kernel<K_, S_, T_, XL_>,                                  \
                              hipFuncAttributeMaxDynamicSharedMemorySize, (int)kLdsLimit);                        \
    hipLaunchKernelGGL((wfae_cln_fwd_kernel<K_, S_, T_, XL_>), dim3(N), dim3(kThreads), lds, st, x, w, bias,      \
                       gamma, beta, y, xhat, mean, rstd, s);                                                      \
  } while (0)
#define WFAE_CLN_FX(K_, S_, T_)            \
  do {                                     \
    if (xl) WFAE_CLN_F(K_, S_, T_, true);  \
    else WFAE_CLN_F(K_, S_, T_, false);    \
  } while (0)
  if (kind == 0) WFAE_CLN_FX(3, 1, false);
  else if (kind == 1) WFAE_CLN_FX(4, 2, false);
  else WFAE_CLN_FX(4, 2, true);
#undef WFAE_CLN_FX
#undef WFAE_CLN_F
  return check_launch("cln_fwd");
}

int wfae_cln_bwd(const float* dy, const float* xhat, const float* rstd, const float* gamma, const float* beta,
                 const float* x, const float* w, float* dx, float* dw, float* dbias, float* dgamma, float* dbeta,
                 int kind, int N, int Cin, int Cout, int H, int W, float slope, void* ws, size_t ws_bytes,
                 wfae_stream_t stream) {
  WFAE_REQUIRE(dy && xhat && rstd && gamma && beta && x && w && dw && dbias && dgamma && dbeta, WFAE_ERR_NULL_POINTER,
               "cln_bwd: null pointer");
  ClnShape s;
  int rc = cln_shape("cln_bwd", kind, N, Cin, Cout, H, W, slope, &s);
  if (rc) return rc;
  const int KK = cln_kk(kind), E = Cout * s.Ho * s.Wo, nW = Cout * Cin * KK;
  const size_t fixed = 18 * sizeof(double) + ((size_t)pad4(E) + (dx ? (size_t)KK * Cin * pad4(Cout) : 0)) * sizeof(float);
  const size_t nX = (size_t)Cin * H * W * sizeof(float);
  // output-row slices of the weight gradient: as many as there are threads for, then as many as LDS has room for
  int nslices = kThreads / (Cin * KK);
  if (nslices < 1) nslices = 1;
  if (nslices > s.Ho) nslices = s.Ho;
  bool xl = fixed + nX <= kLdsLimit;
  auto slice_bytes = [&](int ns) { return ns > 1 ? (size_t)ns * nW * sizeof(float) : (size_t)0; };
  while (nslices > 1 && fixed + (xl ? nX : 0) + slice_bytes(nslices) > kLdsLimit) --nslices;
  const size_t lds = fixed + (xl ? nX : 0) + slice_bytes(nslices);
  WFAE_REQUIRE(lds <= kLdsLimit, WFAE_ERR_UNSUPPORTED, "cln_bwd: %zu bytes of LDS > %zu", lds, kLdsLimit);
  const size_t need = cln_ws_bytes(kind, N, Cin, Cout);
  WFAE_REQUIRE(ws && ws_bytes >= need, WFAE_ERR_WORKSPACE, "cln_bwd: workspace too small (%zu < %zu)", ws_bytes, need);
  float* dwp = (float*)ws;
  float* dbp = dwp + (size_t)N * nW;
  hipStream_t st = (hipStream_t)stream;
#define WFAE_CLN_B(K_, S_, T_, XL_)                                                                               \
  do {                                                                                                            \
    (void)hipFuncSetAttribute((const void*)wfae_cln_bwd_sample_kernel<K_, S_, T_, XL_>,                           \
                              hipFuncAttributeMaxDynamicSharedMemorySize, (int)kLdsLimit);                        \
    hipLaunchKernelGGL((wfae_cln_bwd_sample_kernel<K_, S_, T_, XL_>), dim3(N), dim3(kThreads), lds, st, dy, xhat, \
                       rstd, gamma, beta, x, w, dx, dwp, dbp, s, nslices);                                        \
  } while (0)
#define WFAE_CLN_BX(K_, S_, T_)            \
  do {                                     \
    if (xl) WFAE_CLN_B(K_, S_, T_, true);  \
    else WFAE_CLN_B(K_, S_, T_, false);    \
  } while (0)
  if (kind == 0) WFAE_CLN_BX(3, 1, false);
  else if (kind == 1) WFAE_CLN_BX(4, 2, false);
  else WFAE_CLN_BX(4, 2, true);
#undef WFAE_CLN_BX
#undef WFAE_CLN_B
  if ((rc = check_launch("cln_bwd_sample"))) return rc;
  hipLaunchKernelGGL(wfae_cln_bwd_final_kernel, dim3(cdiv((int64_t)E + nW + Cout, 256)), dim3(256), 0, st, dy, xhat,
                     gamma, beta, dwp, dbp, dgamma, dbeta, dw, dbias, N, E, nW, Cout, slope);
  return check_launch("cln_bwd_final");
}

}  // extern "C"
