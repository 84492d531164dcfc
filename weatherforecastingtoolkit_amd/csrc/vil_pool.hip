// vil_pool.hip — the loader's third conversion kernel: frame stride + block pooling fused into the uint8 'NHWT' -> fp32
// 'NTHW' conversion.  mode 0 (max) is the reference's offline sevir_lr recipe (pipeline/datasets/sevire/sevir.py:575-616:
// frames [::ft], then skimage block_reduce(np.max) with zero padding), mode 1 (mean) its runtime downsample_data_dict
// (:849-890: frames [::ft], then avg_pool2d, remainder dropped).  include/wfae.h states the arithmetic; the tests hold the
// kernels to it bit for bit, so every product, sum and quotient of the mean is rounded on its own (__fmul_rn / __fadd_rn /
// __fdiv_rn: no fma, no reciprocal).
//
// Unlike its two neighbours this kernel reads more than it writes (2 x 3 x 3: up to 18 bytes in for 4 out), so the read is
// the side that is laid out.  Three kernels:
//   rows    T == 1, identity geometry, fw <= 4.  A raw row is W contiguous bytes; a thread owns 4 consecutive outputs and
//           reads the 4 * fw consecutive bytes under them per raw row, as fw dwords where W % 4 == 0 and src is 4-byte
//           aligned, as bytes otherwise (and at a ragged right edge).
//   staged  T > 1, identity geometry.  A raw pixel is T contiguous bytes of which every ft-th is used; a workgroup stages
//           the fh contiguous row segments under 64 outputs in LDS with 16-byte loads (bytes for an unaligned head and
//           tail: the row pitch W * T need not be a multiple of anything) and reduces from there.
//   direct  everything else, and always with transform rows (a rotated line has no contiguous segment): each thread
//           gathers its block's bytes, as augment.hip gathers its pixel.
// Stores: 16-byte nontemporal where Wo % 4 == 0 and dst is 16-byte aligned, dword otherwise.
#include <stdlib.h>
#include <string.h>

#include "common.h"

namespace wfae {

__device__ __forceinline__ float vil_value(uint8_t b, float scale, float offset) {
  return __fmul_rn(scale, __fadd_rn((float)b, offset));
}

// one output from the block of raw pixels [r0, r0 + nr) x [c0, c0 + nc) of sample plane `sp` (H x W x T bytes) at frame t
template <int MODE>
__device__ __forceinline__ float pool_block(const uint8_t* __restrict__ sp, int W, int T, int t, int r0, int nr, int c0,
                                            int nc, float scale, float offset, float count) {
  if constexpr (MODE == 0) {
    unsigned m = 0;
    for (int a = 0; a < nr; ++a) {
      const uint8_t* __restrict__ p = sp + ((long)(r0 + a) * W + c0) * T + t;
      for (int b = 0; b < nc; ++b) m = max(m, (unsigned)p[(long)b * T]);
    }
    return vil_value((uint8_t)m, scale, offset);
  } else {
    float acc = 0.f;
    for (int a = 0; a < nr; ++a) {
      const uint8_t* __restrict__ p = sp + ((long)(r0 + a) * W + c0) * T + t;
      for (int b = 0; b < nc; ++b) acc = __fadd_rn(acc, vil_value(p[(long)b * T], scale, offset));
    }
    return __fdiv_rn(acc, count);
  }
}

// direct gather.  VEC = 4: a thread owns outputs (i, 4q .. 4q+3) (Wo % 4 == 0, dst 16-byte aligned); VEC = 1: one output
template <int VEC, int MODE, bool AUG>
__global__ __launch_bounds__(256) void vil_pool_direct_kernel(const uint8_t* __restrict__ src, const float* __restrict__ xf,
                                                              float* __restrict__ dst, int NB, int H, int W, int T, int ft,
                                                              int fh, int fw, int To, int Ho, int Wo, float scale,
                                                              float offset) {
  const int WQ = Wo / VEC;
  const long idx = (long)blockIdx.x * 256 + threadIdx.x;
  if (idx >= (long)Ho * WQ) return;
  const int i = (int)(idx / WQ), j = (int)(idx - (long)i * WQ) * VEC;
  const long plane = (long)Ho * Wo;
  const float count = (float)((long)fh * fw);                    // (float)(fh * fw): the mean has fh * fw <= H * W
  for (int n = blockIdx.y; n < NB; n += gridDim.y) {
    int blk[VEC];
    if constexpr (AUG) {
      const float* __restrict__ row = xf + (long)n * 4;          // wave-uniform
      const float c = row[0], s = row[1];
      const bool hflip = row[2] != 0.f, vflip = row[3] != 0.f;
#pragma unroll
      for (int k = 0; k < VEC; ++k) blk[k] = aug_src_pixel(i, j + k, Ho, Wo, c, s, hflip, vflip);
    } else {
#pragma unroll
      for (int k = 0; k < VEC; ++k) blk[k] = i * Wo + j + k;
    }
    int r0[VEC], nr[VEC], c0[VEC], nc[VEC];
#pragma unroll
    for (int k = 0; k < VEC; ++k) {
      const int b = blk[k] < 0 ? 0 : blk[k];
      const int bi = b / Wo, bj = b - bi * Wo;
      r0[k] = bi * fh;                                           // < H: bi <= Ho - 1 and (Ho - 1) * fh < H
      c0[k] = bj * fw;
      nr[k] = min(fh, H - r0[k]);
      nc[k] = min(fw, W - c0[k]);
    }
    const uint8_t* __restrict__ sp = src + (long)n * H * W * T;
    float* __restrict__ dp = dst + (long)n * To * plane + (long)i * Wo + j;
    for (int tp = 0; tp < To; ++tp) {
      float v[VEC];
#pragma unroll
      for (int k = 0; k < VEC; ++k) {
        v[k] = blk[k] < 0 ? 0.f : pool_block<MODE>(sp, W, T, tp * ft, r0[k], nr[k], c0[k], nc[k], scale, offset, count);
      }
      if constexpr (VEC == 4) {
        const wfae_vf4 o = {v[0], v[1], v[2], v[3]};
        __builtin_nontemporal_store(o, reinterpret_cast<wfae_vf4*>(dp + (long)tp * plane));
      } else {
        __builtin_nontemporal_store(v[0], dp + (long)tp * plane);
      }
    }
  }
}

// T == 1, identity geometry: a thread owns outputs (i, 4q .. 4q+3) and reads the 4 * FW bytes under them per raw row.
// ST4: one 16-byte store (Wo % 4 == 0, dst 16-byte aligned), else up to four dword stores.  dwords: W % 4 == 0 and src
// 4-byte aligned, so that every full segment starts on a dword.
template <int FW, int MODE, bool ST4>
__global__ __launch_bounds__(256) void vil_pool_rows_kernel(const uint8_t* __restrict__ src, float* __restrict__ dst, int NB,
                                                            int H, int W, int fh, int Ho, int Wo, int dwords, float scale,
                                                            float offset) {
  const int WQ = (Wo + 3) / 4;
  const long idx = (long)blockIdx.x * 256 + threadIdx.x;
  if (idx >= (long)Ho * WQ) return;
  const int i = (int)(idx / WQ), j = (int)(idx - (long)i * WQ) * 4;
  const int r0 = i * fh, nr = min(fh, H - r0);
  const long c0 = (long)j * FW;                                  // < W + 4 * FW
  const int nc = (int)min((long)(4 * FW), (long)W - c0);         // bytes of the segment inside the row, >= 1
  const float count = (float)((long)fh * FW);
  for (int n = blockIdx.y; n < NB; n += gridDim.y) {
    const uint8_t* __restrict__ p = src + ((long)n * H + r0) * W + c0;
    unsigned m[4] = {0, 0, 0, 0};
    float acc[4] = {0.f, 0.f, 0.f, 0.f};
    for (int a = 0; a < nr; ++a, p += W) {
      uint8_t by[4 * FW];
      if (dwords && nc == 4 * FW) {
#pragma unroll
        for (int d = 0; d < FW; ++d) {
          const unsigned w = __builtin_nontemporal_load(reinterpret_cast<const unsigned*>(p) + d);
          by[4 * d] = (uint8_t)w, by[4 * d + 1] = (uint8_t)(w >> 8), by[4 * d + 2] = (uint8_t)(w >> 16),
                 by[4 * d + 3] = (uint8_t)(w >> 24);
        }
      } else {
#pragma unroll
        for (int c = 0; c < 4 * FW; ++c) by[c] = c < nc ? p[c] : (uint8_t)0;   // 0: neutral for the max; the mean never
      }                                                                        // stores an output with a byte outside
#pragma unroll
      for (int k = 0; k < 4; ++k) {
#pragma unroll
        for (int b = 0; b < FW; ++b) {
          if constexpr (MODE == 0) m[k] = max(m[k], (unsigned)by[k * FW + b]);
          else acc[k] = __fadd_rn(acc[k], vil_value(by[k * FW + b], scale, offset));
        }
      }
    }
    float v[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) v[k] = MODE == 0 ? vil_value((uint8_t)m[k], scale, offset) : __fdiv_rn(acc[k], count);
    float* __restrict__ dp = dst + ((long)n * Ho + i) * Wo + j;
    if constexpr (ST4) {
      const wfae_vf4 o = {v[0], v[1], v[2], v[3]};
      __builtin_nontemporal_store(o, reinterpret_cast<wfae_vf4*>(dp));
    } else {
#pragma unroll
      for (int k = 0; k < 4; ++k)
        if (j + k < Wo) __builtin_nontemporal_store(v[k], dp + k);
    }
  }
}

// T > 1, identity geometry: workgroup (i, segment of kStageJ outputs) stages the fh raw row segments under its outputs —
// each one contiguous run of bytes — in LDS, then every thread reduces (frame, output) pairs with the output index fastest,
// so that a wave's stores are 256 contiguous bytes.  A staged byte keeps its global address modulo 16, so full 16-byte
// chunks move as one load and one LDS write whatever the row pitch; the chunk holding the head or the tail of the segment
// moves byte by byte and nothing outside the segment is read.
constexpr int kStageJ = 64;
inline long stage_pitch(int fw, int T) { return (((long)kStageJ * fw * T + 15 + 15) / 16) * 16; }

template <int MODE>
__global__ __launch_bounds__(256) void vil_pool_staged_kernel(const uint8_t* __restrict__ src, float* __restrict__ dst, int NB,
                                                              int H, int W, int T, int ft, int fh, int fw, int To, int Ho,
                                                              int Wo, int pitch, float scale, float offset) {
  extern __shared__ __attribute__((aligned(16))) uint8_t lds[];
  const int nseg = (Wo + kStageJ - 1) / kStageJ;
  const int i = blockIdx.x / nseg, j0 = (blockIdx.x - i * nseg) * kStageJ;
  const int nj = min(kStageJ, Wo - j0);
  const int r0 = i * fh, nr = min(fh, H - r0);
  const int px0 = j0 * fw;                                       // < W
  const int npx = (int)min((long)nj * fw, (long)W - px0);
  const int seg = npx * T;                                       // bytes per staged row, <= pitch - 15
  const float count = (float)((long)fh * fw);
  const long plane = (long)Ho * Wo;
  for (int n = blockIdx.y; n < NB; n += gridDim.y) {
    for (int a = 0; a < nr; ++a) {
      const uint8_t* __restrict__ g = src + (((long)n * H + r0 + a) * W + px0) * T;
      const int mis = (int)((uintptr_t)g & 15);
      const uint8_t* __restrict__ g0 = g - mis;                  // 16-byte aligned; only [g, g + seg) is dereferenced
      uint8_t* __restrict__ l = lds + a * pitch;                 // byte k of the segment lives at l[mis + k]
      const int nchunk = (mis + seg + 15) / 16;
      for (int c = threadIdx.x; c < nchunk; c += 256) {
        const int lo = max(16 * c, mis), hi = min(16 * c + 16, mis + seg);
        if (hi - lo == 16) {
          *reinterpret_cast<wfae_vu4*>(l + 16 * c) =
              __builtin_nontemporal_load(reinterpret_cast<const wfae_vu4*>(g0 + 16 * c));
        } else {
          for (int k = lo; k < hi; ++k) l[k] = g0[k];
        }
      }
    }
    __syncthreads();
    for (int item = threadIdx.x; item < To * kStageJ; item += 256) {
      const int jj = item % kStageJ, tp = item / kStageJ;
      if (jj >= nj) continue;
      const int nc = min(fw, W - (px0 + jj * fw));               // >= 1
      const int t = tp * ft;
      unsigned m = 0;
      float acc = 0.f;
      for (int a = 0; a < nr; ++a) {
        const int mis = (int)((uintptr_t)(src + (((long)n * H + r0 + a) * W + px0) * T) & 15);
        const uint8_t* __restrict__ l = lds + a * pitch + mis + jj * fw * T + t;
        for (int b = 0; b < nc; ++b) {
          if constexpr (MODE == 0) m = max(m, (unsigned)l[b * T]);
          else acc = __fadd_rn(acc, vil_value(l[b * T], scale, offset));
        }
      }
      const float v = MODE == 0 ? vil_value((uint8_t)m, scale, offset) : __fdiv_rn(acc, count);
      __builtin_nontemporal_store(v, dst + ((long)n * To + tp) * plane + (long)i * Wo + j0 + jj);
    }
    __syncthreads();                                             // the next sample overwrites the rows
  }
}

// WFAE_VIL_POOL_STAGED=0 sends T > 1 to the direct gather (tools/vil_pool_bench.py times one against the other); read on
// every call, a getenv costs nothing next to a launch
static bool staged_enabled() {
  const char* e = getenv("WFAE_VIL_POOL_STAGED");
  return !(e && strcmp(e, "0") == 0);
}

template <int MODE>
static void launch_rows(int fw, bool st4, dim3 grid, hipStream_t st, const uint8_t* src, float* dst, int NB, int H, int W,
                        int fh, int Ho, int Wo, int dwords, float scale, float offset) {
#define WFAE_ROWS(FW)                                                                                                   \
  case FW:                                                                                                              \
    if (st4)                                                                                                            \
      hipLaunchKernelGGL((vil_pool_rows_kernel<FW, MODE, true>), grid, dim3(256), 0, st, src, dst, NB, H, W, fh, Ho, Wo, \
                         dwords, scale, offset);                                                                        \
    else                                                                                                                \
      hipLaunchKernelGGL((vil_pool_rows_kernel<FW, MODE, false>), grid, dim3(256), 0, st, src, dst, NB, H, W, fh, Ho,   \
                         Wo, dwords, scale, offset);                                                                    \
    break;
  switch (fw) {
    WFAE_ROWS(1)
    WFAE_ROWS(2)
    WFAE_ROWS(3)
    WFAE_ROWS(4)
  }
#undef WFAE_ROWS
}

template <int MODE, bool AUG>
static void launch_direct(bool st4, int gy, hipStream_t st, const uint8_t* src, const float* xf, float* dst, int NB, int H,
                          int W, int T, int ft, int fh, int fw, int To, int Ho, int Wo, float scale, float offset) {
  if (st4)
    hipLaunchKernelGGL((vil_pool_direct_kernel<4, MODE, AUG>), dim3(cdiv((long)Ho * (Wo / 4), 256), gy), dim3(256), 0, st,
                       src, xf, dst, NB, H, W, T, ft, fh, fw, To, Ho, Wo, scale, offset);
  else
    hipLaunchKernelGGL((vil_pool_direct_kernel<1, MODE, AUG>), dim3(cdiv((long)Ho * Wo, 256), gy), dim3(256), 0, st, src,
                       xf, dst, NB, H, W, T, ft, fh, fw, To, Ho, Wo, scale, offset);
}

}  // namespace wfae

using namespace wfae;

extern "C" {

int wfae_vil_pool_u8_to_f32(const uint8_t* src, const float* xf, float* dst, int NB, int H, int W, int T, int ft, int fh,
                            int fw, int mode, float scale, float offset, wfae_stream_t stream) {
  WFAE_REQUIRE(src && dst, WFAE_ERR_NULL_POINTER, "vil_pool_u8_to_f32: null pointer");
  WFAE_REQUIRE(NB > 0 && H > 0 && W > 0 && T > 0, WFAE_ERR_BAD_SHAPE, "vil_pool_u8_to_f32: bad shape");
  WFAE_REQUIRE(ft > 0 && fh > 0 && fw > 0, WFAE_ERR_BAD_SHAPE, "vil_pool_u8_to_f32: factors (%d, %d, %d) must be >= 1", ft,
               fh, fw);
  WFAE_REQUIRE(mode == 0 || mode == 1, WFAE_ERR_UNSUPPORTED, "vil_pool_u8_to_f32: mode %d (0 = max, 1 = mean)", mode);
  WFAE_REQUIRE(mode == 0 || (fh <= H && fw <= W), WFAE_ERR_BAD_SHAPE,
               "vil_pool_u8_to_f32: mean over %d x %d blocks of a %d x %d frame", fh, fw, H, W);
  WFAE_REQUIRE((long)H * W <= 0x7fffffffL, WFAE_ERR_BAD_SHAPE, "vil_pool_u8_to_f32: frame of %d x %d pixels", H, W);
  const int To = (T - 1) / ft + 1;
  const int Ho = mode == 0 ? (H - 1) / fh + 1 : H / fh, Wo = mode == 0 ? (W - 1) / fw + 1 : W / fw;
  const int gy = NB < 65535 ? NB : 65535;
  const bool st4 = Wo % 4 == 0 && ((uintptr_t)dst & 15) == 0;
  hipStream_t st = (hipStream_t)stream;
  if (xf) {
    if (mode == 0) launch_direct<0, true>(st4, gy, st, src, xf, dst, NB, H, W, T, ft, fh, fw, To, Ho, Wo, scale, offset);
    else launch_direct<1, true>(st4, gy, st, src, xf, dst, NB, H, W, T, ft, fh, fw, To, Ho, Wo, scale, offset);
  } else if (T == 1 && fw <= 4) {
    const int dwords = W % 4 == 0 && ((uintptr_t)src & 3) == 0;
    const dim3 grid(cdiv((long)Ho * ((Wo + 3) / 4), 256), gy);
    if (mode == 0) launch_rows<0>(fw, st4, grid, st, src, dst, NB, H, W, fh, Ho, Wo, dwords, scale, offset);
    else launch_rows<1>(fw, st4, grid, st, src, dst, NB, H, W, fh, Ho, Wo, dwords, scale, offset);
  } else if (T > 1 && (long)fw * T <= 768 && fh * stage_pitch(fw, T) <= 48 * 1024 && staged_enabled()) {
    // fw * T is tested first: the pitch and every LDS offset then fit an int with room to spare
    const int pitch = (int)stage_pitch(fw, T);
    const dim3 grid((unsigned)((long)Ho * cdiv(Wo, kStageJ)), gy);
    if (mode == 0)
      hipLaunchKernelGGL(vil_pool_staged_kernel<0>, grid, dim3(256), (size_t)fh * pitch, st, src, dst, NB, H, W, T, ft, fh,
                         fw, To, Ho, Wo, pitch, scale, offset);
    else
      hipLaunchKernelGGL(vil_pool_staged_kernel<1>, grid, dim3(256), (size_t)fh * pitch, st, src, dst, NB, H, W, T, ft, fh,
                         fw, To, Ho, Wo, pitch, scale, offset);
  } else {
    if (mode == 0) launch_direct<0, false>(st4, gy, st, src, xf, dst, NB, H, W, T, ft, fh, fw, To, Ho, Wo, scale, offset);
    else launch_direct<1, false>(st4, gy, st, src, xf, dst, NB, H, W, T, ft, fh, fw, To, Ho, Wo, scale, offset);
  }
  return check_launch("vil_pool_u8_to_f32");
}

}  // extern "C"
