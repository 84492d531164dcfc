// latent_cache.hip — the two streaming kernels of the latent cache of the frozen AutoencoderKL provider
// (experiments/v1_experiments/_latents.py `LatentCache`).  A row is one frame's payload of L fp32 values: the posterior mode
// (L = C h w) of a `sample: false` provider, the moments (L = 2 C h w) of a `sample: true` one.
//
// scatter: rows of a freshly encoded batch go to their slots of the table; a slot of -1 (the table is full) skips the row.
// gather:  the (B, T) output frames are read from the table (index >= 0) or from the rows encoded this step (index < 0:
//   row -1 - index of `fresh`).  mode 0 copies the row; mode 1 reads moments and writes mean + std * noise with the
//   expression and operand order of aekl_posterior_seq_kernel (aekl.hip), so its bits are that kernel's.
// Both are grid-stride loops of 256 threads, one 16-byte access per operand when the row length allows it (VEC = 4: a group
// of four never crosses a row, nor the mean / logvar boundary), scalar otherwise.  Plain vector loads and stores, no
// atomics; a row is written by exactly one thread group, so two launches give the same bits.
// The host checks slots and indices on the copies it built them from; the kernels still never follow a slot or an index
// outside its array (such a row is skipped).
#include "common.h"

using namespace wfae;

namespace {

template <int VEC>
__global__ __launch_bounds__(256) void latent_scatter_kernel(const float* __restrict__ src, const int* __restrict__ slots,
                                                             float* __restrict__ table, long L, int capacity, long total) {
  const long stride = (long)gridDim.x * blockDim.x * VEC;
  for (long i = ((long)blockIdx.x * blockDim.x + threadIdx.x) * VEC; i < total; i += stride) {
    const long m = i / L, r = i - m * L;
    const int s = slots[m];
    if (s < 0 || s >= capacity) continue;
    float* dst = table + (long)s * L + r;
    if constexpr (VEC == 4)
      *reinterpret_cast<float4*>(dst) = *reinterpret_cast<const float4*>(src + i);
    else
      *dst = src[i];
  }
}

// the source row of output frame f, or null for an index outside [-M, capacity)
__device__ __forceinline__ const float* latent_row(const float* table, const float* fresh, int idx, long L, int capacity, int M) {
  if (idx >= 0) return idx < capacity ? table + (long)idx * L : nullptr;
  const int j = -1 - idx;
  return j < M ? fresh + (long)j * L : nullptr;
}

template <int VEC>
__global__ __launch_bounds__(256) void latent_gather_kernel(const float* __restrict__ table, const float* __restrict__ fresh,
                                                            const int* __restrict__ index, float* __restrict__ out, long L,
                                                            int capacity, int M, long total) {
  const long stride = (long)gridDim.x * blockDim.x * VEC;
  for (long i = ((long)blockIdx.x * blockDim.x + threadIdx.x) * VEC; i < total; i += stride) {
    const long f = i / L, r = i - f * L;
    const float* row = latent_row(table, fresh, index[f], L, capacity, M);
    if (!row) continue;
    if constexpr (VEC == 4)
      *reinterpret_cast<float4*>(out + i) = *reinterpret_cast<const float4*>(row + r);
    else
      out[i] = row[r];
  }
}

template <int VEC>
__global__ __launch_bounds__(256) void latent_gather_sample_kernel(const float* __restrict__ table, const float* __restrict__ fresh,
                                                                   const int* __restrict__ index, const float* __restrict__ noise,
                                                                   float* __restrict__ out, int B, int T, long CHW, int capacity,
                                                                   int M, long total) {
  const long stride = (long)gridDim.x * blockDim.x * VEC;
  for (long i = ((long)blockIdx.x * blockDim.x + threadIdx.x) * VEC; i < total; i += stride) {
    const long f = i / CHW, r = i - f * CHW;
    const long b = f / T, t = f - b * T;
    const float* row = latent_row(table, fresh, index[f], 2 * CHW, capacity, M);
    if (!row) continue;
    const float* pm = row + r;
    const float* pn = noise + (t * B + b) * CHW + r;
    if constexpr (VEC == 4) {
      const float4 mu = *reinterpret_cast<const float4*>(pm);
      const float4 lr = *reinterpret_cast<const float4*>(pm + CHW);
      const float4 nz = *reinterpret_cast<const float4*>(pn);
      float4 o;
      o.x = fmaf(expf(0.5f * fminf(fmaxf(lr.x, -30.0f), 20.0f)), nz.x, mu.x);
      o.y = fmaf(expf(0.5f * fminf(fmaxf(lr.y, -30.0f), 20.0f)), nz.y, mu.y);
      o.z = fmaf(expf(0.5f * fminf(fmaxf(lr.z, -30.0f), 20.0f)), nz.z, mu.z);
      o.w = fmaf(expf(0.5f * fminf(fmaxf(lr.w, -30.0f), 20.0f)), nz.w, mu.w);
      *reinterpret_cast<float4*>(out + i) = o;
    } else {
      const float lv = fminf(fmaxf(pm[CHW], -30.0f), 20.0f);
      const float sd = expf(0.5f * lv);
      out[i] = fmaf(sd, *pn, *pm);
    }
  }
}

inline unsigned stream_grid(long items) {      // 8 blocks per CU; grid-stride beyond
  const long blocks = (items + 255) / 256;
  return (unsigned)(blocks < 2048 ? blocks : 2048);
}

inline bool aligned16(const void* a, const void* b, const void* c, const void* d) {
  return ((uintptr_t)a | (uintptr_t)b | (uintptr_t)c | (uintptr_t)d) % 16 == 0;
}

}  // namespace

extern "C" {

int wfae_latent_scatter(const float* src, const int* slots, float* table, int M, int L, int capacity, wfae_stream_t stream) {
  WFAE_REQUIRE(src && slots && table, WFAE_ERR_NULL_POINTER, "latent_scatter: null pointer");
  WFAE_REQUIRE(M > 0 && L > 0 && capacity > 0, WFAE_ERR_BAD_SHAPE, "latent_scatter: bad shape M=%d L=%d capacity=%d", M, L, capacity);
  const long total = (long)M * L;
  WFAE_REQUIRE(total < (1l << 39) && (long)capacity * L < (1l << 39), WFAE_ERR_BAD_SHAPE, "latent_scatter: too large");
  const bool vec = L % 4 == 0 && aligned16(src, table, nullptr, nullptr);
  const unsigned grid = stream_grid(vec ? total / 4 : total);
  if (vec)
    hipLaunchKernelGGL(latent_scatter_kernel<4>, dim3(grid), dim3(256), 0, (hipStream_t)stream, src, slots, table, (long)L, capacity, total);
  else
    hipLaunchKernelGGL(latent_scatter_kernel<1>, dim3(grid), dim3(256), 0, (hipStream_t)stream, src, slots, table, (long)L, capacity, total);
  return check_launch("latent_scatter");
}

int wfae_latent_gather(const float* table, const float* fresh, const int* index, const float* noise, float* out, int B, int T,
                       int L, int mode, int capacity, int M, wfae_stream_t stream) {
  WFAE_REQUIRE(table && index && out, WFAE_ERR_NULL_POINTER, "latent_gather: null pointer");
  WFAE_REQUIRE(mode == 0 || mode == 1, WFAE_ERR_BAD_SHAPE, "latent_gather: mode %d, expected 0 (copy) or 1 (sample)", mode);
  WFAE_REQUIRE((mode == 1) == (noise != nullptr), WFAE_ERR_NULL_POINTER, "latent_gather: noise belongs to mode 1, and only to it");
  WFAE_REQUIRE(B > 0 && T > 0 && L > 0 && capacity > 0 && M >= 0, WFAE_ERR_BAD_SHAPE,
               "latent_gather: bad shape B=%d T=%d L=%d capacity=%d M=%d", B, T, L, capacity, M);
  WFAE_REQUIRE(mode == 0 || L % 2 == 0, WFAE_ERR_BAD_SHAPE, "latent_gather: mode 1 rows are moments, L=%d is odd", L);
  WFAE_REQUIRE(fresh || M == 0, WFAE_ERR_NULL_POINTER, "latent_gather: M=%d fresh rows without fresh", M);
  const long frames = (long)B * T;
  WFAE_REQUIRE(frames * L < (1l << 39) && (long)capacity * L < (1l << 39) && (long)M * L < (1l << 39), WFAE_ERR_BAD_SHAPE,
               "latent_gather: too large");
  if (mode == 0) {
    const long total = frames * L;
    const bool vec = L % 4 == 0 && aligned16(table, fresh, out, nullptr);
    const unsigned grid = stream_grid(vec ? total / 4 : total);
    if (vec)
      hipLaunchKernelGGL(latent_gather_kernel<4>, dim3(grid), dim3(256), 0, (hipStream_t)stream, table, fresh, index, out, (long)L, capacity, M, total);
    else
      hipLaunchKernelGGL(latent_gather_kernel<1>, dim3(grid), dim3(256), 0, (hipStream_t)stream, table, fresh, index, out, (long)L, capacity, M, total);
  } else {
    const long CHW = L / 2, total = frames * CHW;
    const bool vec = CHW % 4 == 0 && aligned16(table, fresh, out, noise);
    const unsigned grid = stream_grid(vec ? total / 4 : total);
    if (vec)
      hipLaunchKernelGGL(latent_gather_sample_kernel<4>, dim3(grid), dim3(256), 0, (hipStream_t)stream, table, fresh, index, noise, out, B, T, CHW, capacity, M, total);
    else
      hipLaunchKernelGGL(latent_gather_sample_kernel<1>, dim3(grid), dim3(256), 0, (hipStream_t)stream, table, fresh, index, noise, out, B, T, CHW, capacity, M, total);
  }
  return check_launch("latent_gather");
}

}  // extern "C"
