// resae_common.h — the layer kinds of the ae_gan residual autoencoders and their geometry rule, shared by the forward
// (resae.hip) and the backward (resae_bwd.hip).
#pragma once
#include "common.h"

namespace wfae {
namespace resae_geo {

enum { K3S1 = 0, K3S2 = 1, K3UP = 2, K1S1 = 3, K1S2 = 4 };

__host__ __device__ inline int kind_stride(int kind) { return kind == K3S2 || kind == K1S2 ? 2 : 1; }
__host__ __device__ inline int kind_taps(int kind) { return kind >= K1S1 ? 1 : 9; }
__host__ __device__ inline int out_size(int kind, int h) { return kind == K3UP ? 2 * h : kind_stride(kind) == 2 ? (h - 1) / 2 + 1 : h; }

// source index along one axis of output position o through tap k (0..2), or -1 where that is padding
__host__ __device__ inline int src_index(int kind, int o, int k, int h) {
  if (kind == K3UP) {
    const int u = o + k - 1;
    return (u < 0 || u >= 2 * h) ? -1 : (u >> 1);
  }
  const int s = kind_stride(kind) * o + k - 1;
  return (s < 0 || s >= h) ? -1 : s;
}

inline int live_axis(int kind, int k, int h) {
  const int ho = out_size(kind, h);
  for (int o = 0; o < ho; ++o)
    if (src_index(kind, o, k, h) >= 0) return 1;
  return 0;
}

inline int live_mask(int kind, int H, int W) {
  if (kind_taps(kind) == 1) return 1 << 4;
  int m = 0;
  for (int ky = 0; ky < 3; ++ky)
    for (int kx = 0; kx < 3; ++kx)
      if (live_axis(kind, ky, H) && live_axis(kind, kx, W)) m |= 1 << (ky * 3 + kx);
  return m;
}

}  // namespace resae_geo
}  // namespace wfae
