// c1ws.hip — the two passes of a Bottleneck's backward that read the block's input x [NB][C][HW] in FRONT of the first BatchNorm's
// sums at C <= 256, in ONE pass over x (fp32 tensors, fp32 precision with the split GEMMs on, C in {128, 256}, M = C / 4):
//   dW1[m][c]  = sum over images and pixels  dT1[img][m][p] * gelu(x[img][c][p] * scale[c] + shift[c])          (c1w.hip's product)
//   sums[c]    = sum dU, sum dU xhat,  dU = dA1 gelu'(x scale + shift),  dA1 = W1^T dT1,  xhat = (x - mean) invstd
//                                                                             (c1r.hip's sums-alone form, wfae_c1r_bnred(da = NULL))
// Both kernels read x and dT1, evaluate the same gelu_tail_f of u = x scale + shift and split dT1 into its three bf16 planes.
// This is c1wd.hip's construction with the wide and the narrow tensor swapped and an elementwise epilogue added: the loop (a
// K-step of 32 pixels, two LDS stages, global loads two K-steps ahead, one block barrier per K-step), the off_row image, the
// split-K chunking of c1w_chunks and slab_reduce are c1wd_kernel's.  P = x (C rows, activated in the loader), Q = dT1 (M rows).
//   * dW1 is c1w_kernel<float, TM, 1, 1>'s arithmetic product for product (v_mfma_f32_32x32x16_bf16 on ds_read_b128 row
//     fragments, pixel 16 ks + 8 (lane >> 5) + element, the six plane products smallest terms first, k-slabs and K-steps
//     ascending, the slabs of c1w_chunks reduced in slab order into the transposed dW1): bit-identical to
//     wfae_c1w_bwd_weight with the BatchNorm + GELU prologue.
//   * dA1[c][p] contracts over the ROWS of the dT1 tile (K = M: one or two 32-chunks).  The B fragments come through
//     ds_read_b64_tr_b16 from the Q planes (c1wd's pattern on its P planes); the weight fragments W1^T stay in registers, split
//     once in the prologue (12 registers per 16-row block and chunk).  c1r_kernel's arithmetic: v_mfma_f32_16x16x32_bf16,
//     channel 32 chunk + 8 (lane >> 4) + element, the same order of the six plane products, chunks ascending from a zero
//     accumulator: the dA1 that wfae_c1r_bnred forms, bit for bit.  It never leaves the chip.
//   * the sums are bn_act_bwd_reduce_kernel's quad() on that dA1, taken by the LOADER: a 16-byte piece is four aligned pixels
//     of one channel row.  Every wave owns C / 8 channel rows for the whole launch — it loads them, activates and splits them,
//     computes the dA1 tiles of exactly these rows and passes them to its own loader lanes through a wave-private LDS tile
//     (row stride 36 floats: the four row groups of an accumulator write 64 distinct banks).  Writer and readers are the same
//     wave, LDS serves a wave's instructions in order: no block barrier beyond the loop's one.  gelu and gelu' share the
//     tail (one v_rcp, one v_exp); gelu' and xhat of the piece wait in registers from the iteration that activates K-step
//     s + 1 to the next one, where its dA1 exists (dA1 and the sums come first in an iteration, then the next activation:
//     one set of 8 registers per piece is live).  fp32 sums of four, everything above in fp64: two accumulators per piece
//     over the whole K loop, the 8 lanes of a row added at the end, one partial row per workgroup.
//   * C = 128: 4 dW1 tiles of 32 x 32: waves 0-3 carry them, every wave its dA1 rows, each form in its own copy of the loop on
//     a wave-uniform branch (the same number of block barriers in both).  C = 256: 8 tiles of 64 x 32, every wave one.
//     One workgroup per CU in both forms (136 / 242 registers, 78 / 156 KiB of LDS, no scratch).
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
typedef unsigned u32x4 __attribute__((ext_vector_type(4)));
typedef unsigned u32x2 __attribute__((ext_vector_type(2)));

struct C1WSP {
  const float* x;            // [NB][C][HW]
  const float* dt;           // [NB][M][HW]
  const float* w1;           // [M][C]
  const float* scale;        // folded BatchNorm scale / shift, batch mean, invstd of x's channels [C]
  const float* shift;
  const float* mean;
  const float* invstd;
  float* slab;               // [NB * cpi][C][M]
  double* part0;             // [NB * cpi][C] sum dU
  double* part1;             // [NB * cpi][C] sum dU xhat
  int HW;                    // % 32 == 0
  int cpi;                   // K chunks per image
  int kc;                    // pixels per chunk (multiple of 32)
};

constexpr int SNT = 512, SBK = 32;
constexpr int D_LD = 36;     // floats per row of the dA1 tile: 4 rows apart = 16 banks apart

// c1w.hip's row image: 64-byte rows of 32 bf16, 16-byte chunk c of row r at chunk c ^ ((r >> 2) & 3)
__device__ __forceinline__ unsigned off_row(int r, int c) { return (unsigned)(r * 64 + ((c ^ ((r >> 2) & 3)) << 4)); }

__device__ __forceinline__ void split_pair(float a, float b, unsigned& h, unsigned& m, unsigned& l) {
  h = pack_bf16(a, b);
  const float ra = a - bf16_lo(h), rb = b - bf16_hi(h);
  m = pack_bf16(ra, rb);
  l = pack_bf16(ra - bf16_lo(m), rb - bf16_hi(m));
}

template <int C>
__global__ __launch_bounds__(SNT, 2) void c1ws_kernel(C1WSP p) {
  constexpr bool RCST = C == 128;             // the BatchNorm constants of a piece in registers (C = 256: fetched from the lane that holds them)
  constexpr int M = C / 4;
  constexpr int TM = C / 128;                 // dW1: 32-row tiles of x per wave
  constexpr int WQ = M / 32;                  // dW1: waves along the rows of dT1
  constexpr int NDW = 4 * WQ;                 // waves that carry dW1 tiles
  constexpr bool BOTH = NDW == 8;
  constexpr int KCH = M / 32;                 // dA1: 32-row chunks of dT1
  constexpr int RW = C / 8;                   // channel rows a wave owns
  constexpr int RB = RW / 16;                 // dA1: 16-row blocks per wave
  constexpr int LPR = 8;                      // 16-byte loads per row and K-step
  constexpr int P_IT = RW / 8;                // pieces of x per lane and K-step: row RW wave + 8 j + (lane >> 3), pixels 4 (lane & 7) .. + 3
  constexpr int Q_LD = M * LPR;
  static_assert(Q_LD <= SNT, "loader");
  constexpr int A_PLANE_B = C * 64, B_PLANE_B = M * 64;
  constexpr int A_STAGE_B = 3 * A_PLANE_B, STAGE_B = 3 * (A_PLANE_B + B_PLANE_B);
  constexpr int D_WAVE_B = RW * D_LD * 4;
  static_assert(2 * STAGE_B + 8 * D_WAVE_B <= 156 * 1024, "LDS");
  __shared__ __attribute__((aligned(16))) unsigned char smem[2 * STAGE_B + 8 * D_WAVE_B];
  const int t = threadIdx.x, lane = t & 63;
  const int wave = __builtin_amdgcn_readfirstlane(t >> 6);
  const int img = blockIdx.x / p.cpi, chunk = blockIdx.x - img * p.cpi;
  const int k_begin = chunk * p.kc;
  const int k_end = min(p.HW, k_begin + p.kc);
  const int nsteps = (k_end - k_begin) / SBK;
  const bool do_dw = BOTH || wave < NDW;

  // ---- loaders.  x: the wave's own rows; dT1: c1w_kernel's (thread t covers row t / 8, pixels 4 (t % 8) .. + 3)
  const int l_r = lane >> 3, l_e = lane & 7;
  const int row0 = RW * wave;
  const float* Pb = p.x + (long)img * C * p.HW + k_begin;
  const float* Qb = p.dt + (long)img * M * p.HW + k_begin;
  const float* p_src = Pb + (long)(row0 + l_r) * p.HW + l_e * 4;   // piece j: 8 j rows further
  const long p_step = 8l * p.HW;
  // off_row(row0 + 8 j + l_r, l_e >> 1) + 8 (l_e & 1) from piece 0's: 8 rows further = 512 bytes and, for odd j, bit 1 of the swizzle
  const unsigned p_dst0 = off_row(row0 + l_r, l_e >> 1) + (unsigned)((l_e & 1) * 8);
  auto p_dst = [&](int j) { return (p_dst0 ^ (unsigned)(32 * (j & 1))) + 512u * (unsigned)j; };
  // the BatchNorm constants {scale, shift, mean, invstd} of the wave's rows.  C = 128: those of the lane's two pieces in registers.
  // C = 256 (four pieces: 16 more registers spill at the 256 budget): lane i holds those of row row0 + (i & 31) and a piece fetches its row's through
  // ds_bpermute_b32 (the LDS crossbar, no LDS memory).  Not a table in LDS: it made the allocation the whole 160 KiB of a CU (two
  // workgroups of 80 KiB at C = 128) and entries of it then read wrong in some workgroups of a launch
  f32x4 rc[RCST ? P_IT : 1];
  if constexpr (RCST) {
#pragma unroll
    for (int j = 0; j < P_IT; ++j) {
      const int r = row0 + 8 * j + l_r;
      rc[j] = f32x4{p.scale[r], p.shift[r], p.mean[r], p.invstd[r]};
    }
  } else {
    const int r = row0 + (lane & (RW - 1));
    rc[0] = f32x4{p.scale[r], p.shift[r], p.mean[r], p.invstd[r]};
  }
  const bool q_on = Q_LD == SNT || t < Q_LD;
  const int q_r = q_on ? t / LPR : 0, q_e = t % LPR;
  const float* q_src = Qb + (long)q_r * p.HW + q_e * 4;
  const unsigned q_dst = off_row(q_r, q_e >> 1) + (unsigned)((q_e & 1) * 8);
  u32x4 rp[P_IT], rq;
  float gp[P_IT][4], xh[P_IT][4];   // gelu'(u) and xhat of the piece activated last: K-step s + 1 until the sums of iteration s + 1
  double sum1[P_IT], sum2[P_IT];
#pragma unroll
  for (int j = 0; j < P_IT; ++j) sum1[j] = sum2[j] = 0.0;
  auto load_global = [&]() {
#pragma unroll
    for (int j = 0; j < P_IT; ++j) rp[j] = *reinterpret_cast<const u32x4*>(p_src + j * p_step);
    if (q_on) rq = *reinterpret_cast<const u32x4*>(q_src);
  };
  auto advance = [&](bool more) {
    p_src += more ? SBK : 0;
    q_src += more ? SBK : 0;
  };
  // four values -> three planes of 8 bytes
  auto put = [&](unsigned char* base, int plane_b, unsigned dst, float v0, float v1, float v2, float v3) {
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
    for (int j = 0; j < P_IT; ++j) {
      const unsigned u0 = rp[j][0], u1 = rp[j][1], u2 = rp[j][2], u3 = rp[j][3];
      const float x0 = __uint_as_float(u0), x1 = __uint_as_float(u1), x2 = __uint_as_float(u2), x3 = __uint_as_float(u3);
      // bn_act_fwd_kernel<GELU>'s arithmetic for the planes, bn_act_bwd_reduce_kernel's for gelu' and xhat: one tail for both
      f32x4 cst;
      if constexpr (RCST) cst = rc[j];
      else {
        const int from = 4 * (8 * j + l_r);
#pragma unroll
        for (int e = 0; e < 4; ++e) {   // (a scalar copy first: a bit cast of an ext-vector ELEMENT expression read element 0)
          const float mine = rc[0][e];
          cst[e] = __int_as_float(__builtin_amdgcn_ds_bpermute(from, __float_as_int(mine)));
        }
      }
      const float a = cst.x, b = cst.y, mu = cst.z, is = cst.w;
      const float w0 = fmaf(x0, a, b), w1 = fmaf(x1, a, b), w2 = fmaf(x2, a, b), w3 = fmaf(x3, a, b);
      gp[j][0] = gelu_grad_f(w0); gp[j][1] = gelu_grad_f(w1); gp[j][2] = gelu_grad_f(w2); gp[j][3] = gelu_grad_f(w3);
      xh[j][0] = (x0 - mu) * is; xh[j][1] = (x1 - mu) * is; xh[j][2] = (x2 - mu) * is; xh[j][3] = (x3 - mu) * is;
      put(s, A_PLANE_B, p_dst(j), gelu_f(w0), gelu_f(w1), gelu_f(w2), gelu_f(w3));
      // C = 128: one piece at a time (interleaved, the temporaries of two tails and splits are live together)
      if constexpr (!BOTH) __builtin_amdgcn_sched_barrier(0);
    }
    if (q_on) {
      const unsigned u0 = rq[0], u1 = rq[1], u2 = rq[2], u3 = rq[3];
      put(s + A_STAGE_B, B_PLANE_B, q_dst, __uint_as_float(u0), __uint_as_float(u1), __uint_as_float(u2), __uint_as_float(u3));
    }
  };

  // ---- dW1 (c1w_kernel's fragments and products): waves as 4 (rows of x) x WQ (rows of dT1), wave tile 32 TM x 32
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

  // ---- dA1 (c1r_kernel's products) of the wave's own rows: tiles (16 rows row0 + 16 rb .., 16 pixels 16 pt ..) of the K-step
  const int n16 = lane & 15, kg = lane >> 4, tq = n16 >> 2, tp = n16 & 3;
  // the weight operand: A[c][m] = w1[m][c], row c = row0 + 16 rb + n16, rows of dT1 32 ch + 8 kg .. + 7, split as c1r_kernel splits its
  // LDS image
  bf16x8 wa[RB][KCH][3];
#pragma unroll
  for (int rb = 0; rb < RB; ++rb)
#pragma unroll
    for (int ch = 0; ch < KCH; ++ch) {
      const float* src = p.w1 + (long)(32 * ch + 8 * kg) * C + row0 + 16 * rb + n16;
      float v[8];
#pragma unroll
      for (int e = 0; e < 8; ++e) v[e] = src[e * C];
      u32x4 h, m, l;
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        unsigned qh, qm, ql;
        split_pair(v[2 * e], v[2 * e + 1], qh, qm, ql);
        h[e] = qh; m[e] = qm; l[e] = ql;
      }
      wa[rb][ch][0] = __builtin_bit_cast(bf16x8, h);
      wa[rb][ch][1] = __builtin_bit_cast(bf16x8, m);
      wa[rb][ch][2] = __builtin_bit_cast(bf16x8, l);
    }
  __builtin_amdgcn_sched_barrier(0);   // the weights are split before the first tile's loads and activation start
  // transposed reads (c1wd_kernel's): lane 4 tq + tp of group kg addresses row 32 ch + 8 kg + 4 hf + tq of dT1, pixels 16 pt + 4 tp .. + 3
  // and receives rows 8 kg + 4 hf .. + 3 of pixel 16 pt + n16
  // off_row(8 kg + 4 hf + tq, 2 pt + (tp >> 1)) + 8 (tp & 1) from the offset of (pt, hf) = (0, 0): hf moves the row by 4 (256 bytes, bit 0
  // of the swizzle), pt bit 1 of the chunk — one register instead of four across the loop
  const unsigned tr_rd0 = off_row(8 * kg + tq, tp >> 1) + 8u * (unsigned)(tp & 1);
  auto tr_rd = [&](int pt, int hf) { return (tr_rd0 ^ (unsigned)(16 * hf + 32 * pt)) + 256u * (unsigned)hf; };
  unsigned char* const dtile = smem + 2 * STAGE_B + wave * D_WAVE_B;   // this wave's [RW][D_LD] floats
  float* const d_wr = reinterpret_cast<float*>(dtile) + (4 * kg) * D_LD + n16;
  const unsigned char* const d_rd = dtile + (l_r * D_LD + 4 * l_e) * 4;
  auto da_step = [&](int buf) {
    const unsigned char* s = smem + buf * STAGE_B + A_STAGE_B;
    constexpr int PA[6] = {2, 0, 1, 1, 0, 0}, PB[6] = {0, 2, 1, 0, 1, 0};
#pragma unroll
    for (int pt = 0; pt < 2; ++pt) {
      bf16x8 b[KCH][3];
#pragma unroll
      for (int ch = 0; ch < KCH; ++ch)
#pragma unroll
        for (int pl = 0; pl < 3; ++pl) {
          s16x4 part[2];
#pragma unroll
          for (int hf = 0; hf < 2; ++hf)
            part[hf] = __builtin_amdgcn_ds_read_tr16_b64_v4i16(
                (s16x4 __attribute__((address_space(3)))*)(s + pl * B_PLANE_B + ch * (32 * 64) + tr_rd(pt, hf)));
          b[ch][pl] = __builtin_bit_cast(bf16x8, __builtin_shufflevector(part[0], part[1], 0, 1, 2, 3, 4, 5, 6, 7));
        }
#pragma unroll
      for (int rb = 0; rb < RB; ++rb) {
        f32x4 d = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int ch = 0; ch < KCH; ++ch)
#pragma unroll
          for (int pr = 0; pr < 6; ++pr) d = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wa[rb][ch][PA[pr]], b[ch][PB[pr]], d, 0, 0, 0);
        // d[q] = dA1[row0 + 16 rb + 4 kg + q][pixel 16 pt + n16]
#pragma unroll
        for (int q = 0; q < 4; ++q) d_wr[(16 * rb + q) * D_LD + 16 * pt] = d[q];
      }
    }
  };
  // bn_act_bwd_reduce_kernel's quad() (c1r_kernel's BNR epilogue) on the piece this lane activated
  auto sums_step = [&]() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
#pragma unroll
    for (int j = 0; j < P_IT; ++j) {
      const f32x4 v = *reinterpret_cast<const f32x4*>(d_rd + j * (8 * D_LD * 4));
      const float d0 = v.x * gp[j][0], d1 = v.y * gp[j][1];
      const float d2 = v.z * gp[j][2], d3 = v.w * gp[j][3];
      const float h0 = xh[j][0], h1 = xh[j][1], h2 = xh[j][2], h3 = xh[j][3];
      const float s1 = (d0 + d1) + (d2 + d3);
      const float s2 = fmaf(d0, h0, d1 * h1) + fmaf(d2, h2, d3 * h3);
      sum1[j] += (double)s1;
      sum2[j] += (double)s2;
    }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");   // the tile is read before the next K-step's dA1 overwrites it
    __builtin_amdgcn_wave_barrier();
  };

  // the whole loop for a wave with (DW) or without dW1 tiles: at C = 128 two copies entered on a wave-uniform branch, the same
  // number of block barriers in both (one after the prologue, one per K-step)
  auto run = [&](auto dwc) {
    constexpr bool DW = decltype(dwc)::value;
    if constexpr (DW) {
#pragma unroll
      for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int q = 0; q < 16; ++q) acc[i][q] = 0.f;
    }
    if (nsteps > 0) {
      Frag f0, f1;
      load_global();
      advance(nsteps > 1);
      store_lds(0);    // K-step 0: its gelu' and xhat wait for iteration 0
      load_global();   // K-step 1 (or 0 again when there is only one: loaded, never stored)
      advance(nsteps > 2);
      __syncthreads();
      for (int st = 0; st < nsteps; ++st) {
        const int cur = st & 1;
        // every read of stage cur lies in front of the barrier: the next iteration overwrites it.  The fragments of dW1 are read
        // behind the elementwise work, not across it (c1w_kernel reads them one k-slab ahead: here they would be live together
        // with the weight fragments, the waiting gelu' / xhat and the split's temporaries; the second wave of the SIMD covers the
        // read); the products keep c1w_kernel's order: k-slab 0, then 1
        da_step(cur);
        sums_step();            // K-step st: consumes gp / xh before store_lds replaces them
        __builtin_amdgcn_sched_barrier(0);
        if (st + 1 < nsteps) store_lds(cur ^ 1);   // K-step st + 1 (uniform: the last iteration has none)
        load_global();          // K-step st + 2
        advance(st + 3 < nsteps);
        __builtin_amdgcn_sched_barrier(0);
        if constexpr (DW && BOTH) {
          read_frag(f0, cur, 0);
          read_frag(f1, cur, 1);
          mfma_frag(f0);
          mfma_frag(f1);
        } else if constexpr (DW) {   // C = 128: one k-slab's fragments at a time (136 registers: three waves per SIMD fit)
          read_frag(f0, cur, 0);
          mfma_frag(f0);
          read_frag(f0, cur, 1);
          mfma_frag(f0);
        }
        __builtin_amdgcn_sched_barrier(0);
        __syncthreads();
        __builtin_amdgcn_sched_barrier(0);
      }
    }
    // ---- epilogue: the partial dW1^T tile of this (image, chunk) into its slab.  Accumulator register q of lane (r31, lh) is
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
  if constexpr (BOTH) run(std::true_type{});
  else if (do_dw) run(std::true_type{});
  else run(std::false_type{});

  // ---- the sums: the 8 lanes of a row in fp64, one entry of the workgroup's partial row per channel
#pragma unroll
  for (int j = 0; j < P_IT; ++j) {
    double e1 = sum1[j], e2 = sum2[j];
#pragma unroll
    for (int o = 1; o < 8; o <<= 1) {
      e1 += __shfl_xor(e1, o, 64);
      e2 += __shfl_xor(e2, o, 64);
    }
    if (l_e == 0) {
      const long at = (long)blockIdx.x * C + row0 + 8 * j + l_r;
      p.part0[at] = e1;
      p.part1[at] = e2;
    }
  }
}

// on by default; WFAE_C1WS=0 at load or wfae_set_c1ws(0) keeps the pair c1r_bnred (sums alone) + c1w
std::atomic<int> g_c1ws{-1};
inline bool c1ws_on() {
  int v = g_c1ws.load(std::memory_order_relaxed);
  if (v < 0) {
    const char* e = getenv("WFAE_C1WS");
    v = (e && e[0] == '0') ? 0 : 1;
    g_c1ws.store(v, std::memory_order_relaxed);
  }
  return v == 1;
}

inline bool al16(const void* q) { return (reinterpret_cast<uintptr_t>(q) & 15) == 0; }

// HW % 64 == 0: the shapes whose sums c1r.hip serves today (the pair this kernel reproduces)
inline bool c1ws_shape_ok(int C, int mid, int HW) { return (C == 128 || C == 256) && mid * 4 == C && HW > 0 && HW % 64 == 0; }

}  // namespace

extern "C" {

int wfae_set_c1ws(int on) {
  g_c1ws.store(on ? 1 : 0, std::memory_order_relaxed);
  return WFAE_OK;
}

int wfae_get_c1ws(void) { return c1ws_on() ? 1 : 0; }

int wfae_c1ws_supported(int C, int mid, int HW) {
  return (c1ws_on() && c1ws_shape_ok(C, mid, HW) && wfae::split_gemm_enabled()) ? 1 : 0;
}

int wfae_c1ws_stat_rows(int C, int mid, int NB, int HW, size_t ws_bytes) {
  int cpi = 0, kc = 0;
  if (!c1ws_shape_ok(C, mid, HW) || NB <= 0 || !c1w_chunks(C, mid, NB, HW, ws_bytes, &cpi, &kc)) return 0;
  return NB * cpi;
}

int wfae_c1ws_bwd(const float* x, const float* dt1, const float* bn_scale, const float* bn_shift, const float* save_mean,
                  const float* save_invstd, const float* w1, float* dw1, double* part, int64_t part_capacity, int* part_rows, int NB,
                  int C, int mid, int HW, int accumulate, void* ws, size_t ws_bytes, wfae_stream_t stream) {
  WFAE_REQUIRE(x && dt1 && bn_scale && bn_shift && save_mean && save_invstd && w1 && dw1 && part && part_rows && ws,
               WFAE_ERR_NULL_POINTER, "c1ws_bwd: null pointer");
  WFAE_REQUIRE(NB > 0 && C > 0 && mid > 0 && HW > 0 && NB <= 65535 && (int64_t)NB * HW < (1ll << 31), WFAE_ERR_BAD_SHAPE,
               "c1ws_bwd: bad shape");
  WFAE_REQUIRE(c1ws_shape_ok(C, mid, HW), WFAE_ERR_UNSUPPORTED,
               "c1ws_bwd: serves C = 128 or 256 with mid = C / 4 and HW %% 64 == 0 (C %d, mid %d, HW %d)", C, mid, HW);
  WFAE_REQUIRE(c1ws_on() && wfae::split_gemm_enabled(), WFAE_ERR_UNSUPPORTED,
               "c1ws_bwd: needs fp32 precision with the split GEMMs on and wfae_set_c1ws(1)");
  WFAE_REQUIRE(al16(x) && al16(dt1), WFAE_ERR_UNSUPPORTED, "c1ws_bwd: x and dt1 must be 16-byte aligned");
  C1WSP p = {};
  p.x = x; p.dt = dt1; p.w1 = w1;
  p.scale = bn_scale; p.shift = bn_shift; p.mean = save_mean; p.invstd = save_invstd;
  p.slab = (float*)ws;
  p.HW = HW;
  // the slabs of wfae_c1w_bwd_weight on the same shape and workspace, finished by the same reduce
  WFAE_REQUIRE(c1w_chunks(C, mid, NB, HW, ws_bytes, &p.cpi, &p.kc), WFAE_ERR_WORKSPACE, "c1ws_bwd: workspace %zu < %zu", ws_bytes,
               (size_t)NB * C * mid * sizeof(float));
  const int rows = NB * p.cpi;   // one partial row per workgroup
  WFAE_REQUIRE(part_capacity >= 2 * (int64_t)rows * C, WFAE_ERR_WORKSPACE, "c1ws_bwd: part holds %lld doubles, needs %lld",
               (long long)part_capacity, (long long)(2 * (int64_t)rows * C));
  *part_rows = rows;
  p.part0 = part;
  p.part1 = part + (long)rows * C;
  hipStream_t st = (hipStream_t)stream;
  const dim3 grid((unsigned)rows), block(SNT);
  if (C == 128) hipLaunchKernelGGL((c1ws_kernel<128>), grid, block, 0, st, p);
  else hipLaunchKernelGGL((c1ws_kernel<256>), grid, block, 0, st, p);
  const int rc = check_launch("c1ws_bwd");
  if (rc) return rc;
  // slab [C][mid] -> dw1 (mid, C): the transpose wfae_c1w_bwd_weight asks for when x is the operand with more rows
  return slab_reduce((const float*)ws, dw1, nullptr, (long)C * mid, mid, rows, accumulate, st, C);
}

}  // extern "C"
