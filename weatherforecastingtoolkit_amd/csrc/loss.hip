// loss.hip — every "big tensor(s) -> one scalar" loss and its pointwise gradient: sigmoid + L1 and plain L1 (the
// autoencoder's reconstruction loss), mean and hinge mean (contperceptual.py:19-23), sum of squares (gradient norms), MSE
// (pretrained_ae_linear_sevir/train.py:67) and Huber (pretrained_ae_convae_sevir/train.py:155 `nn.HuberLoss`).
//
// Forward: one partial-sum kernel over a term functor leaves one fp64 partial per block, one finalize kernel adds the
// partials and applies the factor.  No atomics: two launches give the same bits.  Which elements a thread adds, in which
// order and in how many blocks is part of each entry point's result, so every entry point names its own block count.
// Backward: one grid-stride kernel over a gradient functor.  A new loss is one term functor, one gradient functor and two
// entry points of a few lines.
#include <algorithm>
#include "common.h"

using namespace wfae;

namespace {

constexpr int RT = 256;  // reduction block size

// ---- term functors: operator()(s, a, b) ADDS the term of one element into the thread's fp64 sum itself.  Returning the
// term for the kernel to add would change results: -ffp-contract=on contracts inside one expression only, and
// `s += (double)d * d` is one fp64 FMA only as long as it stays one expression.
// kInputs: how many of the tensors a, b the term reads.  kQuads: a thread takes four consecutive elements per step where
// the pointers are 16-byte aligned.  kStores: the functor replaces `a` by the value the loss leaves in its output tensor.
template <bool SIGMOID>
struct L1Term {   // |r - x| with r = a, or r = sigmoid(a) stored as the reconstruction
  static constexpr int kInputs = 2;
  static constexpr bool kQuads = true, kStores = SIGMOID;
  __device__ __forceinline__ void operator()(double& s, float& a, float x) const {
    if (SIGMOID) a = sigmoid_f(a);
    s += (double)fabsf(a - x);
  }
};
template <bool HINGE>
struct MeanTerm {   // x, or relu(1 + sign * x)
  static constexpr int kInputs = 1;
  static constexpr bool kQuads = false, kStores = false;
  float sign;
  __device__ __forceinline__ void operator()(double& s, float& x, float) const {
    s += HINGE ? (double)fmaxf(1.f + sign * x, 0.f) : (double)x;
  }
};
struct SumsqTerm {
  static constexpr int kInputs = 1;
  static constexpr bool kQuads = false, kStores = false;
  __device__ __forceinline__ void operator()(double& s, float& x, float) const { s += (double)x * x; }
};
struct SqErrTerm {
  static constexpr int kInputs = 2;
  static constexpr bool kQuads = false, kStores = false;
  __device__ __forceinline__ void operator()(double& s, float& a, float b) const {
    const float d = a - b;
    s += (double)d * d;
  }
};
// the value is returned and added in a statement of its own: nothing of it is contracted into the sum
__device__ __forceinline__ double huber_term(float a, float b, float delta) {
  const float d = a - b, ad = fabsf(d);
  return ad <= delta ? 0.5 * (double)d * (double)d : (double)delta * ((double)ad - 0.5 * (double)delta);
}
struct HuberTerm {
  static constexpr int kInputs = 2;
  static constexpr bool kQuads = false, kStores = false;
  float delta;
  __device__ __forceinline__ void operator()(double& s, float& a, float b) const { s += huber_term(a, b, delta); }
};

// part[block] = the block's sum of terms.  QUADS: thread i0 takes elements 4i .. 4i+3 for i = i0, i0 + stride, ..., then
// the tail (n & ~3) + i0, ...; otherwise single elements i0, i0 + stride, ...
template <bool QUADS, class F>
__global__ __launch_bounds__(RT) void loss_part_kernel(F f, const float* __restrict__ a, const float* __restrict__ b,
                                                       float* __restrict__ out, double* __restrict__ part, long n) {
  __shared__ double sm[16];
  const long stride = (long)gridDim.x * blockDim.x;
  long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  double s = 0.0;
  if (QUADS) {
    const long n4 = n >> 2;
    for (; i < n4; i += stride) {
      float4 av = reinterpret_cast<const float4*>(a)[i];
      const float4 bv = F::kInputs == 2 ? reinterpret_cast<const float4*>(b)[i] : make_float4(0.f, 0.f, 0.f, 0.f);
      f(s, av.x, bv.x); f(s, av.y, bv.y); f(s, av.z, bv.z); f(s, av.w, bv.w);
      if (F::kStores) reinterpret_cast<float4*>(out)[i] = av;
    }
    i = (n4 << 2) + (long)blockIdx.x * blockDim.x + threadIdx.x;
  }
  for (; i < n; i += stride) {
    float av = a[i];
    f(s, av, F::kInputs == 2 ? b[i] : 0.f);
    if (F::kStores) out[i] = av;
  }
  const double r = block_sum(s, sm);
  if (threadIdx.x == 0) part[blockIdx.x] = r;
}

// one block: thread t adds part[t], part[t + blockDim], ... in fp64, then the block sum times mul
__global__ void scalar_finalize_kernel(const double* __restrict__ part, long parts, double mul, float* out_f,
                                       double* out_d) {
  __shared__ double sm[16];
  double s = 0.0;
  for (long i = threadIdx.x; i < parts; i += blockDim.x) s += part[i];
  const double r = block_sum(s, sm);
  if (threadIdx.x == 0) {
    if (out_f) out_f[0] = (float)(r * mul);
    if (out_d) out_d[0] = r * mul;
  }
}

// The two block counts of the forward kernels, both about 16 elements to a thread: ceil(floor(n / 16) / 256) and
// ceil(n / 4096).  They are not the same number (n = 4097: 1 and 2 blocks), and the block count enters the bits of the
// sum: each entry point keeps the one it was written with.
inline int blocks_grid16(int64_t n) { return std::min(grid_1d(n, 16), 1024); }   // L1, mean, sum of squares
inline int blocks_cdiv4096(int64_t n) { return std::min(cdiv(n, 4096), 1024); }        // MSE, Huber

// validation, workspace check and both launches of a forward entry point `what`; the result is sum * mul
template <class F>
int reduce_loss(const char* what, bool ptrs, int64_t n, int blocks, F f, const float* a, const float* b, float* store,
                double mul, float* out_f, double* out_d, void* ws, size_t ws_bytes, wfae_stream_t stream) {
  WFAE_REQUIRE(ptrs, WFAE_ERR_NULL_POINTER, "%s: null pointer", what);
  WFAE_REQUIRE(n > 0, WFAE_ERR_BAD_SHAPE, "%s: bad size", what);
  WFAE_REQUIRE(ws && ws_bytes >= (size_t)blocks * sizeof(double), WFAE_ERR_WORKSPACE, "%s: workspace too small", what);
  hipStream_t st = (hipStream_t)stream;
  const bool aligned = ((reinterpret_cast<uintptr_t>(a) | reinterpret_cast<uintptr_t>(b) |
                         reinterpret_cast<uintptr_t>(store)) & 15) == 0;
  if (F::kQuads && aligned)
    hipLaunchKernelGGL((loss_part_kernel<F::kQuads, F>), dim3(blocks), dim3(RT), 0, st, f, a, b, store, (double*)ws, (long)n);
  else
    hipLaunchKernelGGL((loss_part_kernel<false, F>), dim3(blocks), dim3(RT), 0, st, f, a, b, store, (double*)ws, (long)n);
  if (int rc = check_launch(what)) return rc;
  return scalar_finalize((const double*)ws, blocks, mul, out_f, out_d, st, what);
}

// ---- gradient functors: operator()(gv, a, b) = d loss / d a[i] for gv = (upstream gradient) * (the loss's factor)
template <bool SIGMOID>
struct L1Grad {   // gv sign(r - x), times r (1 - r) through the sigmoid
  static constexpr int kInputs = 2;
  __device__ __forceinline__ float operator()(float gv, float r, float x) const {
    const float d = r - x;
    float sg = d > 0.f ? 1.f : (d < 0.f ? -1.f : 0.f);
    if (SIGMOID) sg *= r * (1.f - r);
    return gv * sg;
  }
};
template <bool HINGE>
struct MeanGrad {   // gv, or gv sign [1 + sign * x > 0]
  static constexpr int kInputs = HINGE ? 1 : 0;
  float sign;
  __device__ __forceinline__ float operator()(float gv, float x, float) const {
    return HINGE ? ((1.f + sign * x > 0.f) ? gv * sign : 0.f) : gv;
  }
};
struct SqErrGrad {
  static constexpr int kInputs = 2;
  __device__ __forceinline__ float operator()(float gv, float a, float b) const { return gv * (a - b); }
};
struct HuberGrad {
  static constexpr int kInputs = 2;
  float delta;
  __device__ __forceinline__ float operator()(float gv, float a, float b) const {
    return gv * fminf(fmaxf(a - b, -delta), delta);
  }
};

template <class F>
__global__ __launch_bounds__(256) void loss_grad_kernel(F f, const float* __restrict__ a, const float* __restrict__ b,
                                                        const float* __restrict__ g, float w, float* __restrict__ da,
                                                        long n) {
  const float gv = g[0] * w;
  const long stride = (long)gridDim.x * blockDim.x;
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride)
    da[i] = f(gv, F::kInputs >= 1 ? a[i] : 0.f, F::kInputs == 2 ? b[i] : 0.f);
}

// The kernel is pointwise, so the grid does not enter the bits; the two counts are the ones the entry points were timed with.
inline int blocks_cdiv1024(int64_t n) { return std::min(cdiv(n, 1024), 8192); }   // MSE, Huber; L1 and mean use grid_1d(n)

template <class F>
int grad_loss(const char* what, bool ptrs, int64_t n, int blocks, F f, const float* a, const float* b, const float* g,
              float w, float* da, wfae_stream_t stream) {
  WFAE_REQUIRE(ptrs, WFAE_ERR_NULL_POINTER, "%s: null pointer", what);
  WFAE_REQUIRE(n > 0, WFAE_ERR_BAD_SHAPE, "%s: bad size", what);
  hipLaunchKernelGGL((loss_grad_kernel<F>), dim3(blocks), dim3(256), 0, (hipStream_t)stream, f, a, b, g, w, da, (long)n);
  return check_launch(what);
}

// Huber's own argument; it is looked at after the pointers and the size, as the third check of both entry points
int huber_delta(const char* what, bool ptrs_and_size, float delta) {
  WFAE_REQUIRE(!ptrs_and_size || delta > 0.f, WFAE_ERR_BAD_SHAPE, "%s: delta must be positive (got %g)", what, (double)delta);
  return WFAE_OK;
}

}  // namespace

int wfae::scalar_finalize(const double* part, long parts, double mul, float* out_f, double* out_d, hipStream_t st,
                          const char* what) {
  hipLaunchKernelGGL(scalar_finalize_kernel, dim3(1), dim3(256), 0, st, part, parts, mul, out_f, out_d);
  return check_launch(what);
}

extern "C" {

int wfae_sigmoid_l1_fwd(const float* h, const float* x, float* recon, float* loss, float weight, int64_t n,
                        void* ws, size_t ws_bytes, wfae_stream_t stream) {
  return reduce_loss("sigmoid_l1_fwd", h && x && recon && loss, n, blocks_grid16(n), L1Term<true>{}, h, x, recon,
                     (double)weight / (double)n, loss, nullptr, ws, ws_bytes, stream);
}
int wfae_l1_fwd(const float* recon, const float* x, float* loss, float weight, int64_t n, void* ws,
                size_t ws_bytes, wfae_stream_t stream) {
  return reduce_loss("l1_fwd", recon && x && loss, n, blocks_grid16(n), L1Term<false>{}, recon, x, nullptr,
                     (double)weight / (double)n, loss, nullptr, ws, ws_bytes, stream);
}
int wfae_sigmoid_l1_bwd(const float* recon, const float* x, const float* gloss, float weight, float* dh,
                        int64_t n, wfae_stream_t stream) {
  return grad_loss("sigmoid_l1_bwd", recon && x && gloss && dh, n, grid_1d(n), L1Grad<true>{}, recon, x, gloss,
                   (float)((double)weight / (double)n), dh, stream);
}
int wfae_l1_bwd(const float* recon, const float* x, const float* gloss, float weight, float* drecon, int64_t n,
                wfae_stream_t stream) {
  return grad_loss("l1_bwd", recon && x && gloss && drecon, n, grid_1d(n), L1Grad<false>{}, recon, x, gloss,
                   (float)((double)weight / (double)n), drecon, stream);
}

int wfae_mean_fwd(const float* x, float* out, int64_t n, int hinge, float sign, float weight, void* ws, size_t ws_bytes,
                  wfae_stream_t stream) {
  const double mul = (double)weight / (double)n;
  if (hinge)
    return reduce_loss("mean_fwd", x && out, n, blocks_grid16(n), MeanTerm<true>{sign}, x, nullptr, nullptr, mul,
                       out, nullptr, ws, ws_bytes, stream);
  return reduce_loss("mean_fwd", x && out, n, blocks_grid16(n), MeanTerm<false>{sign}, x, nullptr, nullptr, mul, out,
                     nullptr, ws, ws_bytes, stream);
}
int wfae_mean_bwd(const float* x, const float* gout, float* dx, int64_t n, int hinge, float sign, float weight,
                  wfae_stream_t stream) {
  const float w = (float)((double)weight / (double)n);
  if (hinge)
    return grad_loss("mean_bwd", x && gout && dx, n, grid_1d(n), MeanGrad<true>{sign}, x, nullptr, gout, w, dx, stream);
  return grad_loss("mean_bwd", x && gout && dx, n, grid_1d(n), MeanGrad<false>{sign}, x, nullptr, gout, w, dx, stream);
}

int wfae_sumsq(const float* x, int64_t n, double* out, void* ws, size_t ws_bytes, wfae_stream_t stream) {
  return reduce_loss("sumsq", x && out, n, blocks_grid16(n), SumsqTerm{}, x, nullptr, nullptr, 1.0, nullptr, out, ws,
                     ws_bytes, stream);
}

int wfae_mse_fwd(const float* pred, const float* target, float* loss, int64_t n, void* ws, size_t ws_bytes,
                 wfae_stream_t stream) {
  return reduce_loss("mse_fwd", pred && target && loss, n, blocks_cdiv4096(n), SqErrTerm{}, pred, target, nullptr,
                     1.0 / (double)n, loss, nullptr, ws, ws_bytes, stream);
}
int wfae_mse_bwd(const float* pred, const float* target, const float* gloss, float* dpred, int64_t n,
                 wfae_stream_t stream) {
  return grad_loss("mse_bwd", pred && target && gloss && dpred, n, blocks_cdiv1024(n), SqErrGrad{}, pred, target, gloss,
                   (float)(2.0 / (double)n), dpred, stream);
}

int wfae_huber_fwd(const float* pred, const float* target, float* loss, int64_t n, float delta, void* ws,
                   size_t ws_bytes, wfae_stream_t stream) {
  if (int rc = huber_delta("huber_fwd", pred && target && loss && n > 0, delta)) return rc;
  return reduce_loss("huber_fwd", pred && target && loss, n, blocks_cdiv4096(n), HuberTerm{delta}, pred, target, nullptr,
                     1.0 / (double)n, loss, nullptr, ws, ws_bytes, stream);
}
int wfae_huber_bwd(const float* pred, const float* target, const float* gloss, float* dpred, int64_t n, float delta,
                   wfae_stream_t stream) {
  if (int rc = huber_delta("huber_bwd", pred && target && gloss && dpred && n > 0, delta)) return rc;
  return grad_loss("huber_bwd", pred && target && gloss && dpred, n, blocks_cdiv1024(n), HuberGrad{delta}, pred, target,
                   gloss, (float)(1.0 / (double)n), dpred, stream);
}

}  // extern "C"
