// augment.hip — train-time augmentation of the SEVIR loader (reference pipeline/datasets/sevir/sevir.py:1035-1058:
// RandomHorizontalFlip, RandomVerticalFlip, then torchvision's rotate with its defaults — nearest neighbour, no expand,
// centre of the image, zero fill) fused into the uint8 'NHWT' -> fp32 'NTHW' conversion of the loader contract.
//
// One pass: every output pixel (i, j) of sample n finds its source pixel once — the inverse rotation of the pixel centre
// in fp32, rintf (round half to even, what grid_sample's 'nearest' does), the bounds test on the rounded integers, then the
// flips — and the T frames of that pixel, which are T consecutive source bytes, are converted in a loop.  The kernel is
// bound by its write (4 B out per 1 B in), so the write is the coalesced side: consecutive lanes own consecutive j, one
// 16-byte nontemporal store per thread and frame where W % 4 == 0, one dword store per thread otherwise.  The gather
// along a rotated line re-uses the cache lines its neighbours fetched; a frame is at most 147 KB, no LDS staging.
#include "common.h"

namespace wfae {

// VEC = 4: a thread owns pixels (i, 4q .. 4q+3) (W % 4 == 0, dst 16-byte aligned); VEC = 1: one pixel
template <int VEC>
__global__ __launch_bounds__(256) void vil_augment_kernel(const uint8_t* __restrict__ src, const float* __restrict__ xf,
                                                          float* __restrict__ dst, int NB, int H, int W, int T,
                                                          float scale) {
  const int WQ = W / VEC;
  const long idx = (long)blockIdx.x * 256 + threadIdx.x;
  if (idx >= (long)H * WQ) return;
  const int i = (int)(idx / WQ), j = (int)(idx - (long)i * WQ) * VEC;
  const long plane = (long)H * W;
  for (int n = blockIdx.y; n < NB; n += gridDim.y) {
    const float* __restrict__ row = xf + (long)n * 4;          // wave-uniform
    const float c = row[0], s = row[1];
    const bool hflip = row[2] != 0.f, vflip = row[3] != 0.f;
    const uint8_t* __restrict__ sp = src + (long)n * plane * T;
    float* __restrict__ dp = dst + (long)n * T * plane + (long)i * W + j;
    int off[VEC];
#pragma unroll
    for (int k = 0; k < VEC; ++k) off[k] = aug_src_pixel(i, j + k, H, W, c, s, hflip, vflip);
#pragma unroll 2
    for (int t = 0; t < T; ++t) {
      float v[VEC];
#pragma unroll
      for (int k = 0; k < VEC; ++k) {
        const bool ok = off[k] >= 0;
        const uint8_t b = sp[ok ? (long)off[k] * T + t : 0];
        v[k] = scale * ((ok ? (float)b : 0.f) + 0.f);
      }
      if constexpr (VEC == 4) {
        const wfae_vf4 o = {v[0], v[1], v[2], v[3]};
        __builtin_nontemporal_store(o, reinterpret_cast<wfae_vf4*>(dp + (long)t * plane));
      } else {
        __builtin_nontemporal_store(v[0], dp + (long)t * plane);
      }
    }
  }
}

}  // namespace wfae

using namespace wfae;

extern "C" {

int wfae_vil_augment_u8_to_f32(const uint8_t* src, const float* xf, float* dst, int NB, int H, int W, int T, float scale,
                               wfae_stream_t stream) {
  WFAE_REQUIRE(src && xf && dst, WFAE_ERR_NULL_POINTER, "vil_augment_u8_to_f32: null pointer");
  WFAE_REQUIRE(NB > 0 && H > 0 && W > 0 && T > 0, WFAE_ERR_BAD_SHAPE, "vil_augment_u8_to_f32: bad shape");
  WFAE_REQUIRE((long)H * W <= 0x7fffffffL, WFAE_ERR_BAD_SHAPE, "vil_augment_u8_to_f32: frame of %d x %d pixels", H, W);
  const int gy = NB < 65535 ? NB : 65535;
  if (W % 4 == 0 && ((uintptr_t)dst & 15) == 0) {
    hipLaunchKernelGGL(vil_augment_kernel<4>, dim3(cdiv((long)H * (W / 4), 256), gy), dim3(256), 0, (hipStream_t)stream,
                       src, xf, dst, NB, H, W, T, scale);
  } else {
    hipLaunchKernelGGL(vil_augment_kernel<1>, dim3(cdiv((long)H * W, 256), gy), dim3(256), 0, (hipStream_t)stream, src,
                       xf, dst, NB, H, W, T, scale);
  }
  return check_launch("vil_augment_u8_to_f32");
}

}  // extern "C"
