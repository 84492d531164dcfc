// c1n.hip — the NARROWING 1x1 products of the C >= 512 Bottlenecks (K = C, M = C/4) on fp32 tensors:
//   Y[img][m][p] = sum_k A[m][k] f(X[img][k][p])        m < M, k < K, p < HW
// the C -> C/4 forward with the BatchNorm + GELU prologue f = gelu(x * scale[k] + shift[k]) (A = w, row-major) and the
// C -> C/4 data gradient in front of the third BatchNorm (A[m][k] = w3[k][m], f = identity).
// The loop, the LDS images and the persistent launch are splitgemm.hip's (sgemm3_kernel, BKIND 0, three planes: 256 x 128 x 32
// or 128 x 256 x 32 block tile, 8 waves with 64 x 64 wave tiles, two LDS stages of 72 KiB, global loads two K-steps ahead
// across items, one barrier per K-step).  The MULTIPLY keeps the arithmetic these products had on gemm.hip's PREC == 2 path, so
// that a training step computes what it computed: v_mfma_f32_32x32x16_bf16, per 16-deep slab the six plane products with the
// smallest terms first, k = 16 slab + 8 (lane >> 5) + element, slabs in ascending k — every output element receives the
// same operations in the same order and the results are bit-identical to that kernel's (tests/test_c1n_gpu.py).  The
// 16x16x32 shape of splitgemm.hip was built first: 0.02 - 0.03 ms faster in the prologue forms, other last bits.
// What differs is the way INTO the LDS: both operands arrive as fp32 and every value is activated and split into its three
// exact bf16 planes ONCE per block, by the thread that loaded it, between the global load and the LDS store —
//   * B, the activation [K][HW] of one image: a thread owns 8 (16 with 256 columns) consecutive pixels of one k-row per K-step;
//     gemm.hip's PREC == 2 path kept fp32 in LDS and every wave that shared a value evaluated the GELU and the split again;
//   * A, the weights (0.5 / 1 MB of fp32, L2-resident): split in the loader as well — the entry points that route here
//     (wfae_conv1x1_fwd_bnact, wfae_conv1x1_bwd_data) carry no workspace a pre-pass could write planes to, and a buffer owned
//     by the library would be shared between the streams of a step.  The transposed weight of the data gradient is read
//     with the lanes along m (256-byte segments per k) so that the thread holds the 8 consecutive k of one row chunk.
// Epilogue: plain fp32 stores into NCHW and, for the forward, the BatchNorm sums of the result in the StatRows format of
// wfae_conv1x1_fwd_bnact (fp32 sums of four adjacent pixels — the statistics pass's arithmetic —, fp64 across the 16 lanes
// of a DPP row as in c1r.hip, accumulated in fp64 per wave in LDS over all items of the block, ONE partial row per block).  Columns the
// loader clamped at an image's edge do not enter the sums.  No spin-waits, flags or atomics: the block barrier of the loop is
// the only synchronisation.
#include "common.h"
#include <atomic>
#include <stdlib.h>
#include <type_traits>

using namespace wfae;

namespace {

typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef short s16x4 __attribute__((ext_vector_type(4)));
typedef short s16x8 __attribute__((ext_vector_type(8)));
typedef unsigned u32x4 __attribute__((ext_vector_type(4)));
typedef float f32x4 __attribute__((ext_vector_type(4)));

struct C1NP {
  const float* W;            // AT: A[m][k] = W[k * M + m]; else A[m][k] = W[m * K + k]
  const float* X;            // [NB][K][HW]
  float* Y;                  // [NB][M][HW]
  const float* pro_scale;    // PRO: folded BatchNorm scale / shift of the input channels [K]
  const float* pro_shift;
  double* part0;             // STATS: [gridDim.x][M] sums, one row per block
  double* part1;             // sums of squares
  int HW;                    // % 8 == 0
  int K;                     // % 64 == 0: an even number of K-steps
  int tpi;                   // column tiles per image
  int total;                 // work items: NB * tpi, tile fastest
};

constexpr int CBK = 32, CNT = 512;

// the two LDS images of splitgemm.hip (bank rule: MI355X_MICROARCH.md, LDS): 16-row ds_read_b128 fragments of K-contiguous
// rows, and k-rows of 128 columns for ds_read_b64_tr_b16
__device__ __forceinline__ unsigned off_row16(int r, int c) {
  return (unsigned)(r * 64 + ((c ^ ((0x78 >> (((r >> 2) & 3) << 1)) & 3)) << 4));
}
__device__ __forceinline__ unsigned off_tr16(int k, int ch) {
  return (unsigned)(k * 256 + ((ch ^ (((k & 3) << 2) | ((k >> 2) & 2))) << 4));
}

#define C1N_DPP_F64(v, CTRL)                                                                                     \
  __hiloint2double(__builtin_amdgcn_update_dpp(0, __double2hiint(v), CTRL, 0xf, 0xf, true),                       \
                   __builtin_amdgcn_update_dpp(0, __double2loint(v), CTRL, 0xf, 0xf, true))
__device__ __forceinline__ double row_sum16(double v) {   // lane 15 of every 16-lane DPP row ends up with the row total
  v += C1N_DPP_F64(v, 0x111);
  v += C1N_DPP_F64(v, 0x112);
  v += C1N_DPP_F64(v, 0x114);
  v += C1N_DPP_F64(v, 0x118);
  return v;
}

// the value of lane l ^ 1 / l ^ 2 (DPP quad_perm [1, 0, 3, 2] / [2, 3, 0, 1])
__device__ __forceinline__ float quad_x1(float v) {
  return __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0xB1, 0xf, 0xf, true));
}
__device__ __forceinline__ float quad_x2(float v) {
  return __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0x4E, 0xf, 0xf, true));
}

// two values -> their three exact bf16 planes, packed (a in the low half)
struct Planes3 { unsigned h, m, l; };
__device__ __forceinline__ Planes3 split_pair(float a, float b) {
  Planes3 r;
  r.h = pack_bf16(a, b);
  const float a1 = a - bf16_lo(r.h), b1 = b - bf16_hi(r.h);
  r.m = pack_bf16(a1, b1);
  r.l = pack_bf16(a1 - bf16_lo(r.m), b1 - bf16_hi(r.m));
  return r;
}

// MW: waves along M (4: 256 x 128 block tile for M = 256; 2: 128 x 256 for M = 128); M == 64 MW: one row tile
template <int MW, bool PRO, bool STATS, bool AT, bool PERSIST>
__global__ __launch_bounds__(CNT, 2) void c1n_kernel(C1NP p) {
  constexpr int BM = 64 * MW, NWV = 8 / MW, BN = 64 * NWV;
  constexpr int ABL = BM / 128, NBL = BN / 128;   // 128-row / 128-column pieces of a stage a thread loads
  constexpr int A_PLANE_B = BM * 64, B_PLANE_B = BN * 64;
  constexpr int A_STAGE_B = 3 * A_PLANE_B;
  constexpr int STAGE_B = 3 * (A_PLANE_B + B_PLANE_B);   // 72 KiB
  constexpr int PRO_MAXK = 4 * BM;
  constexpr int PRO_B = PRO ? 2 * PRO_MAXK * 4 : 0;
  constexpr int ST_B = STATS ? 8 * 2 * 64 * 8 : 0;       // per wave: 64 sums, 64 sums of squares (fp64)
  static_assert(2 * STAGE_B + PRO_B + ST_B <= 160 * 1024, "LDS");
  __shared__ __attribute__((aligned(16))) unsigned char smem[2 * STAGE_B + PRO_B + ST_B];
  float* const lsc = reinterpret_cast<float*>(smem + 2 * STAGE_B);   // scale[K] ++ shift[K]
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  double* const lst = reinterpret_cast<double*>(smem + 2 * STAGE_B + PRO_B) + (STATS ? wave * 128 : 0);

  // work items (column tile, image), tile fastest.  Persistent launch: XCD x owns the contiguous run [x W8, (x + 1) W8) and
  // its gridDim.x / 8 workgroups walk it together; classic launch: one item per workgroup
  int item, item_end, per;
  if constexpr (PERSIST) {
    const int xcd = blockIdx.x & 7, slot = blockIdx.x >> 3;
    const int w8 = (p.total + 7) / 8;
    per = gridDim.x >> 3;
    item = xcd * w8 + slot;
    item_end = min(p.total, (xcd + 1) * w8);
    if (item >= item_end) {   // whole workgroup: nobody reaches a barrier; its partial row is zeros
      if constexpr (STATS) {
        for (int m = t; m < BM; m += CNT) {
          p.part0[(long)blockIdx.x * BM + m] = 0.0;
          p.part1[(long)blockIdx.x * BM + m] = 0.0;
        }
      }
      return;
    }
  } else {
    item = blockIdx.x; item_end = item + 1; per = 1;
  }

  if constexpr (PRO) {
    for (int i = t; i < p.K; i += CNT) {
      lsc[i] = p.pro_scale[i];
      lsc[p.K + i] = p.pro_shift[i];
    }
  }
  if constexpr (STATS) {
    for (int i = lane; i < 128; i += 64) lst[i] = 0.0;
  }

  // A loader: row-major weight — thread (row t >> 2 (+ 128), chunk t & 3) reads 8 consecutive k as two 16-byte pieces;
  // transposed weight — thread (row t & 127 (+ 128), chunk t >> 7) reads its 8 k as 8 dwords, the lanes along m
  const int ac = AT ? (t >> 7) : (t & 3), ar = AT ? (t & 127) : (t >> 2);
  const unsigned a_dst = off_row16(ar, ac);
  const int bk = t >> 4, bch = t & 15;
  const unsigned b_dst = off_tr16(bk, bch);
  const unsigned a_step = AT ? 4u * (unsigned)(CBK * BM) : 4u * CBK;
  const unsigned b_step = 4u * (unsigned)(CBK * p.HW);
  const unsigned a_krow = 4u * BM;   // AT: bytes between two k of one row

  // ---- loader cursor: the (item, K-step) the next global loads fetch — up to two K-steps and one item ahead of the multiply
  const char* __restrict__ Ab = reinterpret_cast<const char*>(p.W);
  const char* __restrict__ Bb = nullptr;
  unsigned a_off[ABL], b_off[NBL];
  int ld_next = item;
  int ld_k = 0;
  const int ld_nsteps = p.K / CBK;
  auto set_cursor = [&](int it) {
    const int img = it / p.tpi;
    const int n0_ = (it - img * p.tpi) * BN;
    ld_k = 0;
    Bb = reinterpret_cast<const char*>(p.X + (long)img * p.K * p.HW);
#pragma unroll
    for (int h = 0; h < ABL; ++h)
      a_off[h] = AT ? 4u * (unsigned)((ac * 8) * BM + ar + 128 * h) : 4u * (unsigned)((ar + 128 * h) * p.K + ac * 8);
    // columns beyond the image are clamped to valid ones (their products land where the epilogue neither stores nor sums)
#pragma unroll
    for (int h = 0; h < NBL; ++h) {
      int n = n0_ + 128 * h + bch * 8;
      if (n >= p.HW) n = p.HW - 8;
      b_off[h] = 4u * (unsigned)(bk * p.HW + n);
    }
  };
  f32x4 ra[ABL][2], rb[NBL][2];
  float rs = 1.f, rh = 0.f;   // PRO: scale / shift of the k-row the B registers hold
  auto load_global = [&]() {
#pragma unroll
    for (int h = 0; h < ABL; ++h) {
      if constexpr (AT) {
#pragma unroll
        for (int e = 0; e < 8; ++e) ra[h][e >> 2][e & 3] = *reinterpret_cast<const float*>(Ab + a_off[h] + e * a_krow);
      } else {
        ra[h][0] = *reinterpret_cast<const f32x4*>(Ab + a_off[h]);
        ra[h][1] = *reinterpret_cast<const f32x4*>(Ab + a_off[h] + 16);
      }
    }
#pragma unroll
    for (int h = 0; h < NBL; ++h) {
      rb[h][0] = *reinterpret_cast<const f32x4*>(Bb + b_off[h]);
      rb[h][1] = *reinterpret_cast<const f32x4*>(Bb + b_off[h] + 16);
    }
    if constexpr (PRO) {
      rs = lsc[CBK * ld_k + bk];
      rh = lsc[p.K + CBK * ld_k + bk];
    }
  };
  // after every load_global: one K-step on; past the item's last one the cursor moves to the workgroup's next item (a
  // uniform branch, once per item) or, when there is none, stays on the last K-step (re-loaded, stored to the idle stage,
  // never read)
  auto advance = [&]() {
    if (__builtin_expect(++ld_k < ld_nsteps, 1)) {
#pragma unroll
      for (int h = 0; h < ABL; ++h) a_off[h] += a_step;
#pragma unroll
      for (int h = 0; h < NBL; ++h) b_off[h] += b_step;
    } else if (ld_next < item_end) {
      set_cursor(ld_next);
      ld_next += per;
    } else {
      ld_k = ld_nsteps - 1;
    }
  };
  // activate, split, store: every value of the stage exactly once per block, in four steps — one per group of six MFMAs
  // of an iteration's first half.  256 rows: A piece 0 | B pairs 0, 1 | A piece 1 | B pairs 2, 3; 128 rows: A piece + B pairs
  // 0, 1 | B pairs 2, 3 | B pairs 4, 5 | B pairs 6, 7.  An A piece leaves as three 16-byte stores, two B pairs as three 8-byte
  // stores: no packed plane outlives its step.
  auto split_a = [&](int h, unsigned char* s) {
    const Planes3 q0 = split_pair(ra[h][0][0], ra[h][0][1]), q1 = split_pair(ra[h][0][2], ra[h][0][3]);
    const Planes3 q2 = split_pair(ra[h][1][0], ra[h][1][1]), q3 = split_pair(ra[h][1][2], ra[h][1][3]);
    unsigned char* d = s + a_dst + h * 128 * 64;
    *reinterpret_cast<u32x4*>(d) = u32x4{q0.h, q1.h, q2.h, q3.h};
    *reinterpret_cast<u32x4*>(d + A_PLANE_B) = u32x4{q0.m, q1.m, q2.m, q3.m};
    *reinterpret_cast<u32x4*>(d + 2 * A_PLANE_B) = u32x4{q0.l, q1.l, q2.l, q3.l};
  };
  auto split_b = [&](int h, int half, unsigned char* s) {   // pixels 4 half .. 4 half + 3 of piece h
    f32x4 v = rb[h][half];
    if constexpr (PRO) {   // gemm.hip's bn_gelu4: bn_act_fwd_kernel's arithmetic
#pragma unroll
      for (int e = 0; e < 4; ++e) v[e] = gelu_f(fmaf(v[e], rs, rh));
    }
    const Planes3 q0 = split_pair(v[0], v[1]), q1 = split_pair(v[2], v[3]);
    unsigned char* d = s + A_STAGE_B + b_dst + h * 128 * 64 + 8 * half;
    *reinterpret_cast<uint2*>(d) = make_uint2(q0.h, q1.h);
    *reinterpret_cast<uint2*>(d + B_PLANE_B) = make_uint2(q0.m, q1.m);
    *reinterpret_cast<uint2*>(d + 2 * B_PLANE_B) = make_uint2(q0.l, q1.l);
  };
  auto split_step = [&](int r, int buf) {
    unsigned char* s = smem + buf * STAGE_B;
    if constexpr (ABL == 2) {
      if ((r & 1) == 0) split_a(r >> 1, s);
      else split_b(0, r >> 1, s);
    } else {
      if (r == 0) split_a(0, s);
      split_b(r >> 1, r & 1, s);
    }
  };

  const int wm0 = (wave / NWV) * 64, wn0 = (wave % NWV) * 64;
  const int l31 = lane & 31, lh = lane >> 5, r15 = lane & 15, g4 = lane >> 4, tq = r15 >> 2, tp = r15 & 3;
  // A fragment of a 32-row tile and 16-deep slab s: lane (l31, lh) reads row l31, chunk 2 s + lh = k 16 s + 8 lh .. + 7
  // (+ 32 half * 64 for the other tile: the swizzle only sees (row >> 2) & 3)
  const unsigned a_rd[2] = {off_row16(wm0 + l31, lh), off_row16(wm0 + l31, 2 + lh)};

  typedef float f32x16 __attribute__((ext_vector_type(16)));
  f32x16 acc[2][2];
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;

  struct Grp {
    bf16x8 v[2][3];   // [16-deep slab][plane] of one 32-row / 32-column tile
  };
  auto read_a = [&](Grp& f, int buf, int half) {
    const unsigned char* s = smem + buf * STAGE_B;
#pragma unroll
    for (int sl = 0; sl < 2; ++sl)
#pragma unroll
      for (int pl = 0; pl < 3; ++pl)
        f.v[sl][pl] = *reinterpret_cast<const bf16x8*>(s + pl * A_PLANE_B + a_rd[sl] + 32 * half * 64);
  };
  auto read_b = [&](Grp& f, int buf, int half) {
    const unsigned char* s = smem + buf * STAGE_B + A_STAGE_B;
    // lane 4q+pp of the 16-lane group g4 addresses k-row q, columns 4pp..4pp+3 of a 4 (k) x 16 (n) block and receives the four
    // k of column pp' = its index in the group; group g4 serves columns 16 (g4 & 1) .. + 15 of the 32-column tile and
    // k = 16 slab + 8 lh .. + 7: two blocks
#pragma unroll
    for (int sl = 0; sl < 2; ++sl)
#pragma unroll
      for (int pl = 0; pl < 3; ++pl) {
        s16x4 part[2];
#pragma unroll
        for (int hf = 0; hf < 2; ++hf) {
          const int row = 16 * sl + 8 * lh + 4 * hf + tq;
          const int col = wn0 + 32 * half + 16 * (g4 & 1);   // first column of the group inside the block
          const int ch = ((col & 127) >> 3) + (tp >> 1);
          const unsigned off = (unsigned)((col >> 7) * 32 * 256) + off_tr16(row, ch) + 8u * (tp & 1);
          part[hf] = __builtin_amdgcn_ds_read_tr16_b64_v4i16((s16x4 __attribute__((address_space(3)))*)(s + pl * B_PLANE_B + off));
        }
        const s16x8 v = __builtin_shufflevector(part[0], part[1], 0, 1, 2, 3, 4, 5, 6, 7);
        f.v[sl][pl] = __builtin_bit_cast(bf16x8, v);
      }
  };
  // six MFMAs: the 16-deep slab sl of the 32 x 32 tile (ah, bh) — gemm.hip's PREC == 2 stage, product for product: the same
  // instruction, the same k in the same lane half and element (k = 16 sl + 8 lh + q), the same order of the six plane
  // products (smallest terms first) and of the slabs, so every output element sees the operations the old kernel gave it
  auto half_quadrant = [&](const Grp& a, const Grp& b, int ah, int bh, int sl) {
    f32x16 c = acc[ah][bh];
    c = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a.v[sl][2], b.v[sl][0], c, 0, 0, 0);
    c = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a.v[sl][0], b.v[sl][2], c, 0, 0, 0);
    c = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a.v[sl][1], b.v[sl][1], c, 0, 0, 0);
    c = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a.v[sl][1], b.v[sl][0], c, 0, 0, 0);
    c = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a.v[sl][0], b.v[sl][1], c, 0, 0, 0);
    c = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a.v[sl][0], b.v[sl][0], c, 0, 0, 0);
    acc[ah][bh] = c;
  };
  auto quadrant = [&](const Grp& a, const Grp& b, int ah, int bh) {
    half_quadrant(a, b, ah, bh, 0);
    half_quadrant(a, b, ah, bh, 1);
  };

  Grp A0, A1, B0, B1;
  // one K-step; on entry A0 = A_lo, bx = B_lo of K-step st (stage cur); on exit A0 = A_lo, by_ = B_lo of K-step st + 1.
  // First half: four groups of six MFMAs, each with a quarter of the split (and GELU) arithmetic of K-step st + 1 spread
  // between its MFMAs — left to itself the scheduler puts all of that vector work in front of the first MFMA, and the two
  // waves of a SIMD, which the barrier keeps in step, then leave the matrix pipe idle together.
  auto iter = [&](int st, Grp& bx, Grp& by_) {
    const int cur = st & 1;
    auto group = [&](auto rc) {
      constexpr int r = decltype(rc)::value;
      if (r == 0) read_b(by_, cur, 1);
      if (r == 1) read_a(A1, cur, 1);
      split_step(r, cur ^ 1);         // K-step st + 1 (the last iteration: K-step 0 of the next item, or a stale copy nobody reads)
      if (r == 3) load_global();      // K-step st + 2 (the last two iterations: K-steps 0 and 1 of the next item)
      half_quadrant(A0, r < 2 ? bx : by_, 0, r >> 1, r & 1);
      // vector instructions of this step per MFMA: 5.5 per split value, about 20 more per activated one
      constexpr int na = ABL == 2 ? ((r & 1) == 0 ? 8 : 0) : (r == 0 ? 8 : 0), nb = ABL == 2 ? ((r & 1) ? 4 : 0) : 4;
      constexpr int V = (na * 6 + nb * (PRO ? 26 : 6) + 8 + 5) / 6;
#pragma unroll
      for (int q = 0; q < 6; ++q) {
        __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);   // MFMA
        __builtin_amdgcn_sched_group_barrier(0x002, V, 0);   // VALU
      }
      __builtin_amdgcn_sched_barrier(0);
    };
    group(std::integral_constant<int, 0>{});
    group(std::integral_constant<int, 1>{});
    group(std::integral_constant<int, 2>{});
    group(std::integral_constant<int, 3>{});
    __builtin_amdgcn_sched_barrier(0);
    __syncthreads();
    __builtin_amdgcn_sched_barrier(0);
    read_a(A0, cur ^ 1, 0);
    quadrant(A1, by_, 1, 1);
    read_b(by_, cur ^ 1, 0);
    quadrant(A1, bx, 1, 0);
#pragma unroll
    for (int q = 0; q < 6; ++q) {
      __builtin_amdgcn_sched_group_barrier(0x100, 3, 0);   // DS read
      __builtin_amdgcn_sched_group_barrier(0x008, 4, 0);   // MFMA
    }
    __builtin_amdgcn_sched_barrier(0);
  };

  // ---- prologue of the workgroup's first item
  set_cursor(item);
  ld_next = item + per;
  __syncthreads();   // scale / shift
  load_global();
  advance();
#pragma unroll
  for (int r = 0; r < 4; ++r) split_step(r, 0);
  load_global();
  advance();
  __syncthreads();
  read_a(A0, 0, 0);
  read_b(B0, 0, 0);

  const int nsteps = p.K / CBK;   // even: K-step 0 of every item lies in stage 0 and B0 holds its B_lo
  for (; item < item_end; item += per) {
    const int img = item / p.tpi;
    const int n0 = (item - img * p.tpi) * BN;
    // the cursor moves BETWEEN the iterations: its once-per-item branch must not cut the body of an iteration
    for (int st = 0; st < nsteps; st += 2) {
      iter(st, B0, B1);
      advance();
      iter(st + 1, B1, B0);
      advance();
    }

    // ---- epilogue: accumulator register r of lane (l31, lh) is Y[8 (r >> 2) + 4 lh + (r & 3)][l31] of its 32 x 32 tile
    float* __restrict__ c0 = p.Y + (long)img * BM * p.HW + (long)(wm0 + 4 * lh) * p.HW + n0 + wn0 + l31;
    const bool whole = n0 + BN <= p.HW;
#pragma unroll
    for (int ti = 0; ti < 2; ++ti)
#pragma unroll
      for (int r = 0; r < 16; ++r)
#pragma unroll
        for (int tj = 0; tj < 2; ++tj)
          if (whole || n0 + wn0 + 32 * tj + l31 < p.HW) c0[(long)(32 * ti + 8 * (r >> 2) + (r & 3)) * p.HW + 32 * tj] = acc[ti][tj][r];
    if constexpr (STATS) {
      // chan_reduce_kernel's arithmetic (norm_act.hip), so that the sums agree with the statistics pass over the stored tensor:
      // the fp32 sums of FOUR ADJACENT pixels, (v0 + v1) + (v2 + v3) and fma(v0, v0, v1 v1) + fma(v2, v2, v3 v3), enter the fp64
      // reduction.  The four pixels of a quad sit in the four lanes 4 a .. 4 a + 3: two quad-permute adds (every lane of the
      // quad ends with the same sum; lane 4 a carries the squares in the order above); then fp64 over the lane's two quads,
      // across the 16 lanes of a DPP row (c1r.hip) and the two DPP rows of the 32 columns, lanes 4 a alone contributing.
      bool ok[2];
#pragma unroll
      for (int tj = 0; tj < 2; ++tj) ok[tj] = (l31 & 3) == 0 && (whole || n0 + wn0 + 32 * tj + l31 < p.HW);   // HW % 8 == 0: whole quads
#pragma unroll
      for (int ti = 0; ti < 2; ++ti)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          double e1 = 0.0, e2 = 0.0;
#pragma unroll
          for (int tj = 0; tj < 2; ++tj) {
            const float v = acc[ti][tj][r];
            const float nb = quad_x1(v);                       // the neighbour's value: v1 in lane 4 a, v3 in lane 4 a + 2
            const float t = v + nb, sq = fmaf(v, v, nb * nb);
            const float s1 = t + quad_x2(t), s2 = sq + quad_x2(sq);
            e1 += ok[tj] ? (double)s1 : 0.0;
            e2 += ok[tj] ? (double)s2 : 0.0;
          }
          double d1 = row_sum16(e1), d2 = row_sum16(e2);   // lanes 15 and 31 of the half: the two halves of the row
          d1 += __shfl_xor(d1, 16, 64);
          d2 += __shfl_xor(d2, 16, 64);
          if (l31 == 31) {
            const int m = 32 * ti + 8 * (r >> 2) + 4 * lh + (r & 3);
            lst[m] += d1;
            lst[64 + m] += d2;
          }
        }
    }
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
      for (int j = 0; j < 2; ++j)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;
  }

  if constexpr (STATS) {   // one partial row per block: the NWV waves of a row group in a fixed order
    __syncthreads();
    const double* all = reinterpret_cast<const double*>(smem + 2 * STAGE_B + PRO_B);
    for (int m = t; m < BM; m += CNT) {
      const int wm = m >> 6, r = m & 63;
      double s1 = 0.0, s2 = 0.0;
#pragma unroll
      for (int wn = 0; wn < NWV; ++wn) {
        s1 += all[(wm * NWV + wn) * 128 + r];
        s2 += all[(wm * NWV + wn) * 128 + 64 + r];
      }
      p.part0[(long)blockIdx.x * BM + m] = s1;
      p.part1[(long)blockIdx.x * BM + m] = s2;
    }
  }
}

// on by default; WFAE_C1N=0 at load or wfae_set_c1n(0) keeps the shapes on gemm.hip
std::atomic<int> g_c1n{-1};
inline bool c1n_on() {
  int v = g_c1n.load(std::memory_order_relaxed);
  if (v < 0) {
    const char* e = getenv("WFAE_C1N");
    v = (e && e[0] == '0') ? 0 : 1;
    g_c1n.store(v, std::memory_order_relaxed);
  }
  return v == 1;
}

inline int num_cus8() {
  static const int n = [] {
    int dev = 0, v = 0;
    if (hipGetDevice(&dev) != hipSuccess || hipDeviceGetAttribute(&v, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || v <= 0)
      v = 256;
    return (v + 7) / 8 * 8;
  }();
  return n;
}

template <int MW, bool PRO, bool STATS, bool AT>
void launch_c1n(const C1NP& p, bool persist, int grid, hipStream_t st) {
  if (persist) hipLaunchKernelGGL((c1n_kernel<MW, PRO, STATS, AT, true>), dim3((unsigned)grid), dim3(CNT), 0, st, p);
  else hipLaunchKernelGGL((c1n_kernel<MW, PRO, STATS, AT, false>), dim3((unsigned)grid), dim3(CNT), 0, st, p);
}

}  // namespace

namespace wfae {

// Routed shapes (tools/kbench.py --only c1n, old and new interleaved on one box: profiles/r05_kbench_c1n_vs_gemm.txt)
bool c1n_takes(int M, int K, int HW, bool transposed, bool pro) {
  if (!c1n_on() || !split_gemm_enabled()) return false;
  if (!((M == 128 && K == 512) || (M == 256 && K == 1024))) return false;
  if (HW < 8 || HW % 8 != 0 || (long)K * HW >= (1l << 29)) return false;   // 32-bit byte offsets inside one image
  if (transposed && pro) return false;
  return true;
}

// 1: launched; 0: not served (the caller keeps its own kernel; *stat_rows untouched); < 0: error
int c1n_launch(const float* w, bool transposed, const float* x, const float* scale, const float* shift, float* y, int NB, int K, int M,
               int HW, double* stat_part, int64_t stat_capacity, int* stat_rows, hipStream_t st, const char* what) {
  const bool pro = scale != nullptr, stats = stat_part != nullptr;
  if (!c1n_takes(M, K, HW, transposed, pro) || (transposed && stats)) return 0;
  if (((reinterpret_cast<uintptr_t>(w) | reinterpret_cast<uintptr_t>(x) | reinterpret_cast<uintptr_t>(y)) & 15) != 0) return 0;
  const int bn = M == 256 ? 128 : 256;
  C1NP p = {};
  p.W = w; p.X = x; p.Y = y;
  p.pro_scale = scale; p.pro_shift = shift;
  p.HW = HW; p.K = K;
  p.tpi = cdiv(HW, bn);
  const long total = (long)NB * p.tpi;
  if (total >= (1l << 30)) return 0;
  p.total = (int)total;
  // persistent (one workgroup per CU) when there are more items than CUs; K / 32 is 16 or 32: even
  const bool persist = p.total > num_cus8();
  const int grid = persist ? num_cus8() : p.total;
  if (stats) {
    // one partial row per block; the caller's buffer holds 4 ceil(NB HW / 128) M doubles
    if (stat_capacity < 2 * (int64_t)grid * M) return 0;
    p.part0 = stat_part;
    p.part1 = stat_part + (long)grid * M;
  }
  if (M == 256) {
    if (transposed) launch_c1n<4, false, false, true>(p, persist, grid, st);
    else if (pro && stats) launch_c1n<4, true, true, false>(p, persist, grid, st);
    else if (pro) launch_c1n<4, true, false, false>(p, persist, grid, st);
    else if (stats) launch_c1n<4, false, true, false>(p, persist, grid, st);
    else launch_c1n<4, false, false, false>(p, persist, grid, st);
  } else {
    if (transposed) launch_c1n<2, false, false, true>(p, persist, grid, st);
    else if (pro && stats) launch_c1n<2, true, true, false>(p, persist, grid, st);
    else if (pro) launch_c1n<2, true, false, false>(p, persist, grid, st);
    else if (stats) launch_c1n<2, false, true, false>(p, persist, grid, st);
    else launch_c1n<2, false, false, false>(p, persist, grid, st);
  }
  const int rc = check_launch(what);
  if (rc) return rc;
  if (stats) *stat_rows = grid;
  return 1;
}

}  // namespace wfae

extern "C" {

int wfae_set_c1n(int on) {
  g_c1n.store(on ? 1 : 0, std::memory_order_relaxed);
  return WFAE_OK;
}

int wfae_get_c1n(void) { return c1n_on() ? 1 : 0; }

}  // extern "C"
