// c1wd.hip — the two products of a Bottleneck's backward pass that read the incoming gradient dy [NB][C][HW] at C <= 256, in ONE
// pass over dy (fp32 tensors, fp32 precision with the split GEMMs on, C in {128, 256}, M = C / 4):
//   dW3[c][m]      = sum over images and pixels  dy[img][c][p] * gelu(t2[img][m][p] * scale[m] + shift[m])      (c1w.hip's product)
//   dA3[img][m][p] = sum over c                  w3[c][m] * dy[img][c][p]                                        (c1r.hip's product)
// Both kernels were HBM-bound on dy and each split every dy value into its three bf16 planes.  Here the loop, the LDS image and
// the split-K slabs are c1w.hip's: a K-step is 32 pixels, the dy tile [C rows][32 pixels] and the activated t2 tile [M][32] are
// split ONCE by the thread that loaded them and stored as three exact bf16 planes of pixel-contiguous 64-byte rows (off_row),
// two stages, one block barrier per K-step and no other synchronisation.
//   * dW3 is c1w_kernel's arithmetic product for product — v_mfma_f32_32x32x16_bf16 on ds_read_b128 row fragments, pixel
//     16 ks + 8 (lane >> 5) + element, the six plane products smallest terms first, k-slabs and K-steps ascending, the chunking
//     of c1w_chunks, slab_reduce in slab order: bit-identical to wfae_c1w_bwd_weight (tests/test_c1wd_gpu.py).  Only real
//     rows are multiplied: the 64-row Q tile of c1w_kernel<float, 1, 1, 2> at M = 32 held 32 clamped rows.
//   * dA3 contracts over the ROWS of the same dy tile.  Its B fragments (eight consecutive channels of one pixel per lane)
//     come through ds_read_b64_tr_b16: the 16 lanes of a group address rows 8 g + 4 hf + (i >> 2), pixels 4 (i & 3) .. + 3 of a
//     4-channel x 16-pixel block and lane i receives the four channels of pixel i.  With off_row's swizzle ((row >> 2) & 3 on
//     the 16-byte chunk) the 32 lanes the LDS serves together hit 64 distinct banks (MI355X_MICROARCH.md, LDS): the image
//     serves both read patterns without a conflict.  The weight operand W3^T (M x C) stays in registers: every wave owns one
//     16-row x 16-pixel result tile of the K-step and holds the three-plane fragments of its 16 rows for all C channels
//     (48 registers at C = 128, 96 at C = 256), split once in the prologue.  The arithmetic is c1r_kernel's:
//     v_mfma_f32_16x16x32_bf16, channel 32 chunk + 8 (lane >> 4) + element, the same order of the six plane products, chunks
//     ascending from a zero accumulator: bit-identical to wfae_c1r_fwd with the transposed weight.
//   * C = 128: 4 dW3 tiles of 32 x 32 and 4 dA3 tiles per K-step: waves 0-3 carry dW3, waves 4-7 dA3 (wave w and w + 4 share
//     a SIMD), each role in its own copy of the loop (`run`), 114 registers: two workgroups per CU as c1w runs.  With both
//     roles in one loop the weight fragments and the dW3 fragments are live together (202 registers, one workgroup per CU;
//     84 spilled at the 128 budget); that form, with its loads three K-steps ahead, ran 0.82 ms per launch at 384 x 384
//     against 0.79.  C = 256: 8 + 8 tiles, every wave carries one of each; two 60 KiB stages leave no room for a second
//     workgroup, and the 256-register budget holds the weight fragments (252 used).
#include "common.h"
#include <atomic>
#include <stdlib.h>
#include <type_traits>

using namespace wfae;

namespace {

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef short s16x4 __attribute__((ext_vector_type(4)));
typedef short s16x8 __attribute__((ext_vector_type(8)));
typedef unsigned u32x4 __attribute__((ext_vector_type(4)));
typedef unsigned u32x2 __attribute__((ext_vector_type(2)));

struct C1WDP {
  const float* dy;           // [NB][C][HW]
  const float* t2;           // [NB][M][HW]
  const float* w3;           // [C][M]
  const float* pro_scale;    // folded BatchNorm scale / shift of t2's channels [M]
  const float* pro_shift;
  float* slab;               // [NB * cpi][C][M]
  float* da;                 // [NB][M][HW]
  int HW;                    // % 32 == 0
  int cpi;                   // K chunks per image
  int kc;                    // pixels per chunk (multiple of 32)
};

constexpr int DNT = 512, DBK = 32;

// c1w.hip's row image: 64-byte rows of 32 bf16, 16-byte chunk c of row r at chunk c ^ ((r >> 2) & 3)
__device__ __forceinline__ unsigned off_row(int r, int c) { return (unsigned)(r * 64 + ((c ^ ((r >> 2) & 3)) << 4)); }

__device__ __forceinline__ void split_pair(float a, float b, unsigned& h, unsigned& m, unsigned& l) {
  h = pack_bf16(a, b);
  const float ra = a - bf16_lo(h), rb = b - bf16_hi(h);
  m = pack_bf16(ra, rb);
  l = pack_bf16(ra - bf16_lo(m), rb - bf16_hi(m));
}

template <int C>
__global__ __launch_bounds__(DNT, C == 128 ? 4 : 2) void c1wd_kernel(C1WDP p) {
  constexpr int M = C / 4;
  constexpr int TM = C / 128;                 // dW3: 32-row tiles of dy per wave
  constexpr int WQ = M / 32;                  // dW3: waves along the rows of t2
  constexpr int NDW = 4 * WQ;                 // waves that carry dW3 tiles
  constexpr bool BOTH = NDW == 8;             // every wave carries a dW3 and a dA3 tile
  constexpr int KCH = C / 32;                 // dA3: 32-channel chunks
  constexpr int LPR = 8;                      // 16-byte loads per row and K-step
  constexpr int P_LD = C * LPR, Q_LD = M * LPR;
  constexpr int P_IT = P_LD / DNT;
  static_assert(P_LD % DNT == 0 && Q_LD <= DNT, "loader");
  constexpr int A_PLANE_B = C * 64, B_PLANE_B = M * 64;
  constexpr int A_STAGE_B = 3 * A_PLANE_B, STAGE_B = 3 * (A_PLANE_B + B_PLANE_B);
  __shared__ __attribute__((aligned(16))) unsigned char smem[2 * STAGE_B];
  const int t = threadIdx.x, lane = t & 63;
  const int wave = __builtin_amdgcn_readfirstlane(t >> 6);
  const int img = blockIdx.x / p.cpi, chunk = blockIdx.x - img * p.cpi;
  const int k_begin = chunk * p.kc;
  const int k_end = min(p.HW, k_begin + p.kc);
  const int nsteps = (k_end - k_begin) / DBK;
  const bool do_dw = BOTH || wave < NDW, do_da = BOTH || wave >= NDW;

  // ---- loaders (c1w_kernel's): load j of a thread covers row idx / 8, pixels 4 (idx % 8) .. + 3 of the K-step, idx = t + 512 j
  const float* Pb = p.dy + (long)img * C * p.HW + k_begin;
  const float* Qb = p.t2 + (long)img * M * p.HW + k_begin;
  const float* p_src[P_IT];
  unsigned p_dst[P_IT];
#pragma unroll
  for (int j = 0; j < P_IT; ++j) {
    const int idx = t + j * DNT, r = idx / LPR, e = idx % LPR;
    p_src[j] = Pb + (long)r * p.HW + e * 4;
    p_dst[j] = off_row(r, e >> 1) + (unsigned)((e & 1) * 8);
  }
  const bool q_on = Q_LD == DNT || t < Q_LD;
  const int q_r = q_on ? t / LPR : 0, q_e = t % LPR;
  const float* q_src = Qb + (long)q_r * p.HW + q_e * 4;
  const unsigned q_dst = off_row(q_r, q_e >> 1) + (unsigned)((q_e & 1) * 8);
  const float q_s = p.pro_scale[q_r], q_h = p.pro_shift[q_r];
  u32x4 rp[P_IT], rq;
  auto load_global = [&]() {
#pragma unroll
    for (int j = 0; j < P_IT; ++j) rp[j] = *reinterpret_cast<const u32x4*>(p_src[j]);
    if (q_on) rq = *reinterpret_cast<const u32x4*>(q_src);
  };
  auto advance = [&](bool more) {
#pragma unroll
    for (int j = 0; j < P_IT; ++j) p_src[j] += more ? DBK : 0;
    q_src += more ? DBK : 0;
  };
  // one loaded 16-byte piece -> LDS: 4 values -> (activation) -> three planes of 8 bytes
  auto put = [&](unsigned char* base, int plane_b, unsigned dst, u32x4 r, bool act, float s, float h) {
    const unsigned u0 = r[0], u1 = r[1], u2 = r[2], u3 = r[3];
    float v0 = __uint_as_float(u0), v1 = __uint_as_float(u1), v2 = __uint_as_float(u2), v3 = __uint_as_float(u3);
    if (act) {   // bn_act_fwd_kernel<GELU>'s arithmetic
      v0 = gelu_f(fmaf(v0, s, h)); v1 = gelu_f(fmaf(v1, s, h));
      v2 = gelu_f(fmaf(v2, s, h)); v3 = gelu_f(fmaf(v3, s, h));
    }
    unsigned h0, m0, l0, h1, m1, l1;
    split_pair(v0, v1, h0, m0, l0);
    split_pair(v2, v3, h1, m1, l1);
    *reinterpret_cast<u32x2*>(base + dst) = u32x2{h0, h1};
    *reinterpret_cast<u32x2*>(base + plane_b + dst) = u32x2{m0, m1};
    *reinterpret_cast<u32x2*>(base + 2 * plane_b + dst) = u32x2{l0, l1};
  };
  auto store_lds = [&](int buf) {
    unsigned char* s = smem + buf * STAGE_B;
#pragma unroll
    for (int j = 0; j < P_IT; ++j) put(s, A_PLANE_B, p_dst[j], rp[j], false, 0.f, 0.f);
    if (q_on) put(s + A_STAGE_B, B_PLANE_B, q_dst, rq, true, q_s, q_h);
  };

  // ---- dW3 (c1w_kernel's fragments and products): waves as 4 (rows of dy) x WQ (rows of t2), wave tile 32 TM x 32
  const int wm0 = (BOTH ? (wave >> 1) : (wave & 3)) * (32 * TM), wn0 = BOTH ? (wave & 1) * 32 : 0;
  const int r31 = lane & 31, lh = lane >> 5;
  const unsigned a_rd = (unsigned)((wm0 + r31) * 64), b_rd = (unsigned)((wn0 + r31) * 64);
  const int a_x = (r31 >> 2) & 3;
  f32x16 acc[TM];
  struct Frag {
    bf16x8 a[TM][3], b[3];
  };
  auto read_frag = [&](Frag& f, int buf, int ks) {
    const unsigned char* s = smem + buf * STAGE_B;
    const unsigned a_c = (unsigned)(((2 * ks + lh) ^ a_x) << 4);
#pragma unroll
    for (int i = 0; i < TM; ++i)
#pragma unroll
      for (int pl = 0; pl < 3; ++pl)
        f.a[i][pl] = *reinterpret_cast<const bf16x8*>(s + pl * A_PLANE_B + a_rd + i * (32 * 64) + a_c);
#pragma unroll
    for (int pl = 0; pl < 3; ++pl) f.b[pl] = *reinterpret_cast<const bf16x8*>(s + A_STAGE_B + pl * B_PLANE_B + b_rd + a_c);
  };
  auto mfma_frag = [&](const Frag& f) {
#pragma unroll
    for (int i = 0; i < TM; ++i) {
      f32x16 c = acc[i];   // smallest terms first
      c = __builtin_amdgcn_mfma_f32_32x32x16_bf16(f.a[i][2], f.b[0], c, 0, 0, 0);
      c = __builtin_amdgcn_mfma_f32_32x32x16_bf16(f.a[i][0], f.b[2], c, 0, 0, 0);
      c = __builtin_amdgcn_mfma_f32_32x32x16_bf16(f.a[i][1], f.b[1], c, 0, 0, 0);
      c = __builtin_amdgcn_mfma_f32_32x32x16_bf16(f.a[i][1], f.b[0], c, 0, 0, 0);
      c = __builtin_amdgcn_mfma_f32_32x32x16_bf16(f.a[i][0], f.b[1], c, 0, 0, 0);
      c = __builtin_amdgcn_mfma_f32_32x32x16_bf16(f.a[i][0], f.b[0], c, 0, 0, 0);
      acc[i] = c;
    }
  };

  // ---- dA3 (c1r_kernel's products): tile (16 rows 16 mt .., 16 pixels 16 pt ..) of the K-step; lane (n16, kg) of the MFMA
  const int dtile = BOTH ? wave : (wave & 3);
  const int mt = dtile >> 1, pt = dtile & 1;
  const int n16 = lane & 15, kg = lane >> 4, tq = n16 >> 2, tp = n16 & 3;
  // the weight operand: A[m][k] = w3[k][m], row m = 16 mt + n16, channels 32 ch + 8 kg .. + 7, split as c1r_kernel splits its LDS image
  bf16x8 wa[KCH][3];
  auto load_weights = [&]() {
#pragma unroll
    for (int ch = 0; ch < KCH; ++ch) {
      const float* src = p.w3 + (long)(32 * ch + 8 * kg) * M + 16 * mt + n16;
      float v[8];
#pragma unroll
      for (int e = 0; e < 8; ++e) v[e] = src[e * M];
      u32x4 h, m, l;
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        unsigned qh, qm, ql;
        split_pair(v[2 * e], v[2 * e + 1], qh, qm, ql);
        h[e] = qh; m[e] = qm; l[e] = ql;
      }
      wa[ch][0] = __builtin_bit_cast(bf16x8, h);
      wa[ch][1] = __builtin_bit_cast(bf16x8, m);
      wa[ch][2] = __builtin_bit_cast(bf16x8, l);
    }
  };
  // transposed reads: lane 4 tq + tp of group kg addresses channel row 32 ch + 8 kg + 4 hf + tq, pixels 16 pt + 4 tp .. + 3 (16-byte
  // chunk 2 pt + (tp >> 1), its half tp & 1) and receives channels 8 kg + 4 hf .. + 3 of pixel 16 pt + n16; (row >> 2) & 3 = (2 kg + hf) & 3
  unsigned tr_rd[2];
#pragma unroll
  for (int hf = 0; hf < 2; ++hf) tr_rd[hf] = off_row(8 * kg + 4 * hf + tq, 2 * pt + (tp >> 1)) + 8u * (unsigned)(tp & 1);
  float* const da_dst = p.da + ((long)img * M + 16 * mt + 4 * kg) * p.HW + k_begin + 16 * pt + n16;
  auto da_step = [&](int buf, int st) {
    const unsigned char* s = smem + buf * STAGE_B;
    constexpr int PA[6] = {2, 0, 1, 1, 0, 0}, PB[6] = {0, 2, 1, 0, 1, 0};
    f32x4 d = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int ch = 0; ch < KCH; ++ch) {
      bf16x8 b[3];
#pragma unroll
      for (int pl = 0; pl < 3; ++pl) {
        s16x4 part[2];
#pragma unroll
        for (int hf = 0; hf < 2; ++hf)
          part[hf] = __builtin_amdgcn_ds_read_tr16_b64_v4i16(
              (s16x4 __attribute__((address_space(3)))*)(s + pl * A_PLANE_B + ch * (32 * 64) + tr_rd[hf]));
        b[pl] = __builtin_bit_cast(bf16x8, __builtin_shufflevector(part[0], part[1], 0, 1, 2, 3, 4, 5, 6, 7));
      }
#pragma unroll
      for (int pr = 0; pr < 6; ++pr) d = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wa[ch][PA[pr]], b[PB[pr]], d, 0, 0, 0);
    }
    // d[q] = dA3[16 mt + 4 kg + q][pixel 16 pt + n16]: 16 lanes write 64 contiguous bytes of a row
    float* o = da_dst + 32 * st;
#pragma unroll
    for (int q = 0; q < 4; ++q) o[(long)q * p.HW] = d[q];
  };

  // the whole loop for a wave that carries dW3 tiles (DW), a dA3 tile (DA) or both.  At C = 128 the two roles run as two copies of
  // the loop, entered on a wave-uniform branch: every wave meets the same number of block barriers (one after the prologue, one per
  // K-step) whichever copy it runs, and the registers of a copy are those of its own role — the resident weight fragments of the
  // dA3 waves and the fragments and accumulators of the dW3 waves never share a register file budget
  auto run = [&](auto dwc, auto dac) {
    constexpr bool DW = decltype(dwc)::value, DA = decltype(dac)::value;
    if constexpr (DW) {
#pragma unroll
      for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int q = 0; q < 16; ++q) acc[i][q] = 0.f;
    }
    if constexpr (DA) load_weights();
    if (nsteps > 0) {
      Frag f0, f1;
      load_global();
      advance(nsteps > 1);
      store_lds(0);
      load_global();   // K-step 1 (or 0 again when there is only one: stored to the idle stage, never read)
      advance(nsteps > 2);
      __syncthreads();
      if constexpr (DW) read_frag(f0, 0, 0);
      for (int st = 0; st < nsteps; ++st) {
        const int cur = st & 1;
        if constexpr (DW) read_frag(f1, cur, 1);
        store_lds(cur ^ 1);   // K-step st + 1; in the last iteration a stale copy nobody reads
        load_global();        // K-step st + 2
        advance(st + 3 < nsteps);
        if constexpr (DW) mfma_frag(f0);
        if constexpr (DA) da_step(cur, st);   // every read of stage cur lies in front of the barrier: the next iteration overwrites it
        __builtin_amdgcn_sched_barrier(0);
        __syncthreads();
        __builtin_amdgcn_sched_barrier(0);
        if constexpr (DW) {
          read_frag(f0, cur ^ 1, 0);
          mfma_frag(f1);
        }
        __builtin_amdgcn_sched_barrier(0);
      }
    }
    // ---- epilogue: the partial dW3 tile of this (image, chunk) into its slab.  Accumulator register q of lane (r31, lh) is
    // C[(q & 3) + 8 (q >> 2) + 4 lh][r31] of its 32 x 32 tile: 32 lanes write 128 contiguous bytes of a slab row.
    if constexpr (DW) {
      float* __restrict__ Cb = p.slab + (long)blockIdx.x * C * M;
#pragma unroll
      for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int q = 0; q < 16; ++q) {
          const int row = wm0 + 32 * i + (q & 3) + 8 * (q >> 2) + 4 * lh;
          Cb[(long)row * M + wn0 + r31] = acc[i][q];
        }
    }
  };
  if constexpr (BOTH) run(std::true_type{}, std::true_type{});
  else if (do_dw) run(std::true_type{}, std::false_type{});
  else run(std::false_type{}, std::true_type{});
}

// on by default; WFAE_C1WD=0 at load or wfae_set_c1wd(0) keeps the pair c1w + c1r
std::atomic<int> g_c1wd{-1};
inline bool c1wd_on() {
  int v = g_c1wd.load(std::memory_order_relaxed);
  if (v < 0) {
    const char* e = getenv("WFAE_C1WD");
    v = (e && e[0] == '0') ? 0 : 1;
    g_c1wd.store(v, std::memory_order_relaxed);
  }
  return v == 1;
}

inline bool al16(const void* q) { return (reinterpret_cast<uintptr_t>(q) & 15) == 0; }

// HW % 64 == 0: the shapes whose dA3 c1r.hip serves today (the pair this kernel reproduces)
inline bool c1wd_shape_ok(int C, int mid, int HW) { return (C == 128 || C == 256) && mid * 4 == C && HW > 0 && HW % 64 == 0; }

}  // namespace

extern "C" {

int wfae_set_c1wd(int on) {
  g_c1wd.store(on ? 1 : 0, std::memory_order_relaxed);
  return WFAE_OK;
}

int wfae_get_c1wd(void) { return c1wd_on() ? 1 : 0; }

int wfae_c1wd_supported(int C, int mid, int HW) {
  return (c1wd_on() && c1wd_shape_ok(C, mid, HW) && wfae::split_gemm_enabled()) ? 1 : 0;
}

int wfae_c1wd_bwd(const float* dy, const float* t2, const float* bn_scale, const float* bn_shift, const float* w3, float* dw3,
                  float* da3, int NB, int C, int mid, int HW, int accumulate, void* ws, size_t ws_bytes, wfae_stream_t stream) {
  WFAE_REQUIRE(dy && t2 && bn_scale && bn_shift && w3 && dw3 && da3 && ws, WFAE_ERR_NULL_POINTER, "c1wd_bwd: null pointer");
  WFAE_REQUIRE(NB > 0 && C > 0 && mid > 0 && HW > 0 && NB <= 65535 && (int64_t)NB * HW < (1ll << 31), WFAE_ERR_BAD_SHAPE,
               "c1wd_bwd: bad shape");
  WFAE_REQUIRE(c1wd_shape_ok(C, mid, HW), WFAE_ERR_UNSUPPORTED,
               "c1wd_bwd: serves C = 128 or 256 with mid = C / 4 and HW %% 64 == 0 (C %d, mid %d, HW %d)", C, mid, HW);
  WFAE_REQUIRE(c1wd_on() && wfae::split_gemm_enabled(), WFAE_ERR_UNSUPPORTED,
               "c1wd_bwd: needs fp32 precision with the split GEMMs on and wfae_set_c1wd(1)");
  WFAE_REQUIRE(al16(dy) && al16(t2), WFAE_ERR_UNSUPPORTED, "c1wd_bwd: dy and t2 must be 16-byte aligned");
  C1WDP p = {};
  p.dy = dy; p.t2 = t2; p.w3 = w3;
  p.pro_scale = bn_scale; p.pro_shift = bn_shift;
  p.slab = (float*)ws; p.da = da3;
  p.HW = HW;
  // the slabs of wfae_c1w_bwd_weight on the same shape and workspace, finished by the same reduce
  WFAE_REQUIRE(c1w_chunks(C, mid, NB, HW, ws_bytes, &p.cpi, &p.kc), WFAE_ERR_WORKSPACE, "c1wd_bwd: workspace %zu < %zu", ws_bytes,
               (size_t)NB * C * mid * sizeof(float));
  hipStream_t st = (hipStream_t)stream;
  const dim3 grid((unsigned)(NB * p.cpi)), block(DNT);
  if (C == 128) hipLaunchKernelGGL((c1wd_kernel<128>), grid, block, 0, st, p);
  else hipLaunchKernelGGL((c1wd_kernel<256>), grid, block, 0, st, p);
  const int rc = check_launch("c1wd_bwd");
  if (rc) return rc;
  return slab_reduce((const float*)ws, dw3, nullptr, (long)C * mid, mid, NB * p.cpi, accumulate, st, 0);
}

}  // extern "C"
