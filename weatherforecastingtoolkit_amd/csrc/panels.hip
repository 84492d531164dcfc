// panels.hip — prediction / target / difference panels in the SEVIR VIL colours, drawn where the tensors already are
// (reference pipeline/helpers.py:155-225 `log_wandb_images`: three rows per sample, one column per frame; there through a
// host copy of the whole batch, numpy and a matplotlib figure per sample).  include/wfae.h states the layout and the
// arithmetic; the tests hold the kernel to tests/panels_ref.py byte for byte.
//
// One thread per figure pixel: it finds its row block (target / prediction / difference), its panel and its place inside
// the panel, quantises the one or two source values it needs, looks its colour up in the table it was handed and writes
// three bytes; the thread of a scanline's first pixel also writes the filter byte in front.  Rows are 1 + 3 Wfig bytes,
// so nothing is aligned: byte stores.  A figure is a few MB and drawn a few times per epoch, far from any roof.
#include "common.h"

namespace wfae {

// (uint8)(clamp(x, 0, 1) * 255.0f): one fp32 multiply, then truncation.  NaN fails the first comparison: 0.
__device__ __forceinline__ unsigned panel_quant(float x) {
  const float c = x > 0.f ? (x < 1.f ? x : 1.f) : 0.f;
  return (unsigned)(int)__fmul_rn(c, 255.0f);
}

__global__ __launch_bounds__(256) void panel_render_kernel(const float* __restrict__ pred, const float* __restrict__ target,
                                                           const uint8_t* __restrict__ lut_vil,
                                                           const uint8_t* __restrict__ lut_diff, uint8_t* __restrict__ out,
                                                           int nb, int T, int H, int W, int g, int Hfig, int Wfig) {
  const long idx = (long)blockIdx.x * 256 + threadIdx.x;
  if (idx >= (long)Hfig * Wfig) return;
  const int y = (int)(idx / Wfig), x = (int)(idx - (long)y * Wfig);
  const int rb = y / (H + g), ry = y - rb * (H + g);             // rb <= 2: y < 3 H + 2 g
  const int t = x / (W + g), cx = x - t * (W + g);               // t <= T - 1: x < T W + (T - 1) g
  const bool gap = ry >= H || cx >= W;
  const long row_bytes = 1 + 3 * (long)Wfig;
  const long o = (long)y * row_bytes + 1 + 3 * (long)x;          // < Hfig * row_bytes < 2^31
  for (int n = blockIdx.y; n < nb; n += gridDim.y) {
    unsigned r = 255, gr = 255, b = 255;
    if (!gap) {
      const long src = (((long)n * T + t) * H + ry) * W + cx;
      const uint8_t* __restrict__ c;
      if (rb == 0) c = lut_vil + 3 * panel_quant(target[src]);
      else if (rb == 1) c = lut_vil + 3 * panel_quant(pred[src]);
      else {
        const int ut = (int)panel_quant(target[src]), up = (int)panel_quant(pred[src]);
        c = lut_diff + 3 * (ut > up ? ut - up : up - ut);
      }
      r = c[0], gr = c[1], b = c[2];
    }
    uint8_t* __restrict__ fig = out + (long)n * Hfig * row_bytes;
    if (x == 0) fig[o - 1] = 0;                                  // PNG filter type 0 (None)
    fig[o] = (uint8_t)r, fig[o + 1] = (uint8_t)gr, fig[o + 2] = (uint8_t)b;
  }
}

// elements in [0, 1] (NaN and +-inf fail a comparison): a grid-stride pass leaves one count per workgroup, one workgroup
// adds them in order.  Integers: exact whatever the order.
constexpr int kCountBlocks = 1024;

__global__ __launch_bounds__(256) void range_count_part_kernel(const float* __restrict__ x, long n,
                                                               unsigned long long* __restrict__ part) {
  __shared__ unsigned long long sm[4];
  unsigned long long c = 0;
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long)gridDim.x * 256) {
    const float v = x[i];
    c += (v >= 0.f && v <= 1.f) ? 1u : 0u;
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) c += __shfl_xor(c, o, 64);
  if ((threadIdx.x & 63) == 0) sm[threadIdx.x >> 6] = c;
  __syncthreads();
  if (threadIdx.x == 0) part[blockIdx.x] = sm[0] + sm[1] + sm[2] + sm[3];
}

__global__ __launch_bounds__(64) void range_count_final_kernel(const unsigned long long* __restrict__ part, int parts,
                                                               int64_t* __restrict__ count) {
  unsigned long long c = 0;
  for (int i = threadIdx.x; i < parts; i += 64) c += part[i];
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) c += __shfl_xor(c, o, 64);
  if (threadIdx.x == 0) *count = (int64_t)c;
}

static int count_blocks(int64_t n) {
  const int64_t b = (n + 1023) / 1024;                           // four elements to a thread before the grid strides
  return (int)(b < 1 ? 1 : b > kCountBlocks ? kCountBlocks : b);
}

// bytes of one figure, or 0 where the arguments are refused or the figure reaches 2^31 bytes
static size_t panel_bytes(int T, int H, int W, int g) {
  if (T < 1 || H < 1 || W < 1 || g < 0) return 0;
  const int64_t hfig = 3 * (int64_t)H + 2 * (int64_t)g, wfig = (int64_t)T * W + ((int64_t)T - 1) * g;
  if (hfig > 0x7fffffffLL || wfig > 0x7fffffffLL / 3) return 0;
  const int64_t bytes = hfig * (1 + 3 * wfig);                   // < 2^31 * 2^31: no overflow
  return bytes < (1LL << 31) ? (size_t)bytes : 0;
}

}  // namespace wfae

using namespace wfae;

extern "C" {

size_t wfae_panel_bytes(int T, int H, int W, int g) { return panel_bytes(T, H, W, g); }

int wfae_panel_render(const float* pred, const float* target, const uint8_t* lut_vil, const uint8_t* lut_diff, uint8_t* out,
                      int B, int nb, int T, int H, int W, int g, wfae_stream_t stream) {
  WFAE_REQUIRE(pred && target && lut_vil && lut_diff && out, WFAE_ERR_NULL_POINTER, "panel_render: null pointer");
  WFAE_REQUIRE(B > 0 && T > 0 && H > 0 && W > 0, WFAE_ERR_BAD_SHAPE, "panel_render: bad shape (%d, %d, %d, %d)", B, T, H, W);
  WFAE_REQUIRE(nb >= 1 && nb <= B, WFAE_ERR_BAD_SHAPE, "panel_render: %d samples to draw of a batch of %d", nb, B);
  WFAE_REQUIRE(g >= 0, WFAE_ERR_BAD_SHAPE, "panel_render: gap %d", g);
  WFAE_REQUIRE(panel_bytes(T, H, W, g) > 0, WFAE_ERR_BAD_SHAPE,
               "panel_render: a figure of %d frames of %d x %d with gap %d has 2^31 bytes or more", T, H, W, g);
  const int Hfig = 3 * H + 2 * g, Wfig = T * W + (T - 1) * g;    // both fit: their product is below 2^31 / 3
  const dim3 grid(cdiv((long)Hfig * Wfig, 256), nb < 65535 ? nb : 65535);
  hipLaunchKernelGGL(panel_render_kernel, grid, dim3(256), 0, (hipStream_t)stream, pred, target, lut_vil, lut_diff, out, nb,
                     T, H, W, g, Hfig, Wfig);
  return check_launch("panel_render");
}

size_t wfae_range_count_workspace_bytes(int64_t n) { return n < 1 ? 0 : (size_t)count_blocks(n) * 8; }

int wfae_range_count(const float* x, int64_t n, int64_t* count, void* ws, size_t ws_bytes, wfae_stream_t stream) {
  WFAE_REQUIRE(x && count && ws, WFAE_ERR_NULL_POINTER, "range_count: null pointer");
  WFAE_REQUIRE(n >= 1, WFAE_ERR_BAD_SHAPE, "range_count: %lld elements", (long long)n);
  const int blocks = count_blocks(n);
  WFAE_REQUIRE(ws_bytes >= (size_t)blocks * 8 && ((uintptr_t)ws & 7) == 0, WFAE_ERR_WORKSPACE,
               "range_count: workspace %zu < %zu, or not 8-byte aligned", ws_bytes, (size_t)blocks * 8);
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(range_count_part_kernel, dim3(blocks), dim3(256), 0, st, x, (long)n, (unsigned long long*)ws);
  hipLaunchKernelGGL(range_count_final_kernel, dim3(1), dim3(64), 0, st, (const unsigned long long*)ws, blocks, count);
  return check_launch("range_count");
}

}  // extern "C"
