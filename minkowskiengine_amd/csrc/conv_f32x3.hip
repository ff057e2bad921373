// fp32 sparse convolution (forward / dgrad) on the bf16 matrix pipe of gfx950: every fp32 operand is split
// EXACTLY into three bf16 terms and the product is rebuilt from six v_mfma_f32_16x16x32_bf16 ("bf16x6", the
// 3xTF32 idea with three terms), accumulated in fp32.
//
// Why: an fp32 MFMA (v_mfma_f32_16x16x4_f32, 157 TFLOP/s) blocks its SIMD for every other wave (docs/HISTORY.md 3.1a) and
// k_conv_tile_f32 sits at 0.5 of that peak; the bf16 pipe is 16x faster per product and co-issues with vector
// instructions.  Six bf16 MFMAs per 32 channels cost 96 cycles against 256 for eight fp32 MFMAs.
//
// Arithmetic.  a = a1 + a2 + a3 exactly, where a1 = the upper 16 bits of a's fp32 encoding (a bf16 by truncation),
// a2 = the upper 16 bits of (a - a1), a3 = a - a1 - a2 (at most 8 significant bits are left, so it IS a bf16);
// all subtractions are exact in fp32.  Then  a * b = a1 b1 + (a1 b2 + a2 b1) + (a1 b3 + a2 b2 + a3 b1) + rest,
// |rest| = |a2 b3 + a3 b2 + a3 b3| < 2^-23 |a b|: the dropped terms are below one fp32 rounding of the product.
// bf16 x bf16 products are exact in fp32 and the MFMA accumulates in fp32, so the result differs from an fp32 FMA
// chain by rounding noise of the same order (tests: <= 2e-6 of sum |a b| against float64; the reference operators
// themselves are at 1e-6).  Sums run in the plan's fixed order: bitwise reproducible.  Non-finite inputs: an
// infinity turns into NaN (inf - inf in the split) where fp32 arithmetic would keep the infinity.
//
// Structure: the tile-plan kernel of conv_bf16.hip (target-stationary, fp32 accumulator tile in LDS, single-offset
// batches, heaviest-first tile order) with fp32 rows gathered into registers, split while they are written to the
// three LDS stage planes, and fp32 output.  The reference computes this path in fp32
// (src/convolution_gpu.cu:137-155, AT_DISPATCH_FLOATING_TYPES).
#include <type_traits>
#include <vector>
#include "conv_common.hpp"
#include "conv_ws.hpp"
#include "wgrad_reduce.hpp"

namespace me {


// waves of a workgroup: NC / 16 column blocks x GS group shares (wave = share * (NC / 16) + column block); a share
// takes every GS-th group of a batch, so that narrow column slabs still put two waves on every SIMD
__host__ __device__ constexpr int x3_group_shares(int nc) { return nc >= 96 ? 1 : (nc == 64 ? 2 : 4); }

// accumulator tile + TWO stage buffers (three planes + the target indices of 64 rows each)
__host__ __device__ constexpr int conv_f32x3_lds_bytes(int nc, int kc, int tile_rows) {
  return (tile_rows + 1) * (nc + kAccPad) * 4 + 2 * ME_MAX_BATCH_GROUPS * 16 * (3 * x3_stage_ld(kc) * 2 + 4);
}

// Packed weights: for offset k, source-channel chunk c, 16-column block cb, split plane p (0..2) and 32-channel
// step v, lane (q = lane >> 4, i16 = lane & 15) finds the plane-p terms of
//   W[k][c*KC + v*32 + q*8 + j][cb*16 + i16],  j = 0..7
// as ONE 16-byte element at (((((k*nchunks + c)*ncb + cb)*3 + p)*(KC/32) + v)*64 + lane); zero beyond the real
// channel counts.
template <int KC>
__global__ __launch_bounds__(256) void k_pack_weights_f32x3(const float *__restrict__ w, int c_src, int c_dst,
                                                           int transposed, int nchunks, int ncb,
                                                           u32x4 *__restrict__ wp, int64_t total) {
  constexpr int KS = KC / 32;
  const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;   // one (k, c, cb, v, lane): writes 3 planes
  if (e >= total) return;
  const int lane = (int)(e % 64);
  int64_t r = e / 64;
  const int v = (int)(r % KS);
  r /= KS;
  const int cb = (int)(r % ncb);
  r /= ncb;
  const int c = (int)(r % nchunks);
  const int64_t k = r / nchunks;
  const int q = lane >> 4, i16 = lane & 15;
  const int col = cb * 16 + i16;
  float val[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    const int ch = c * KC + v * 32 + q * 8 + j;
    val[j] = 0.f;
    if (ch < c_src && col < c_dst) {
      // plain: w is [K, c_src, c_dst]; transposed (dgrad): w is the forward kernel [K, c_dst, c_src]
      const int64_t idx = transposed ? (k * c_dst + col) * c_src + ch : (k * c_src + ch) * c_dst + col;
      val[j] = w[idx];
    }
  }
  u32x4 p1, p2, p3;
  split3<true>(f32x4{val[0], val[1], val[2], val[3]}, f32x4{val[4], val[5], val[6], val[7]}, p1, p2, p3);
  const int64_t base = ((((k * nchunks + c) * ncb + cb) * 3) * KS + v) * 64 + lane;
  wp[base] = p1;
  wp[base + (int64_t)KS * 64] = p2;
  wp[base + (int64_t)2 * KS * 64] = p3;
}

// R groups of one offset in one wave: groups share, share + GS, ... of the staged batch, 16 output columns.
// Per 32-channel step and group: the three planes of the rows (3 ds_read_b128, requested one step ahead) and six
// MFMAs, smallest terms first; A = weights, B = rows, so a lane ends with 4 consecutive output columns of one
// target row.  The old accumulator values are requested before the first MFMA and added at the end (rows of a
// single-offset batch are distinct and the columns are wave-private: plain read - add - write, no atomics).
// The operand reads are inline asm with hand-placed waits: left to itself hipcc sinks every ds_read next to the MFMA
// that uses it (ds_read, s_waitcnt lgkmcnt(0), v_mfma, ds_read, ...), which puts one LDS latency in front of almost
// every MFMA — measured 2400 cycles per batch for 768 cycles of MFMAs.  Here all reads of a step are issued back to
// back, one step ahead of the MFMAs that consume them.
template <int R, int GS, int KC>
__device__ __forceinline__ void mma_groups_f32x3(const __bf16 *__restrict__ rowp, const int (&pofs)[KC / 32],
                                                 const bf16x8 (&w)[3][KC / 32], const int32_t *__restrict__ dstp,
                                                 float *__restrict__ accp, int acc_ld) {
  typedef __attribute__((address_space(3))) const char lds_char;
  constexpr int KS = KC / 32;
  constexpr int LD = StageLayout<KC>::kLd;
  constexpr int PLANE = ME_MAX_BATCH_GROUPS * 16 * LD;
  const unsigned row_addr = (unsigned)(uintptr_t)(lds_char *)rowp;   // LDS byte address of this lane's row
  bf16x8 a[2][R][3];
  auto read_step = [&](int s, bf16x8 (&dst)[R][3]) {
    const unsigned addr = row_addr + (unsigned)pofs[s] * 2u;
#pragma unroll
    for (int r = 0; r < R; ++r) {
#pragma unroll
      for (int p = 0; p < 3; ++p)
        asm volatile("ds_read_b128 %0, %1 offset:%2"
                     : "=v"(dst[r][p])
                     : "v"(addr), "n"((p * PLANE + r * GS * 16 * LD) * 2)
                     : "memory");   // (keeps the compiler's own LDS loads / stores on their side of the read: the
                                    // counted waits below assume program order)
    }
  };
  // all LDS operations older than the last `younger` ones have completed; ties the registers so that the MFMAs
  // reading them stay below
  // (the accumulators are tied in as well: the wait of step s + 1 must stay below the MFMAs of step s)
  f32x4 old[R], acc[R];
  auto wait_step = [](bf16x8 (&dst)[R][3], f32x4 (&acc)[R], auto younger) {
#pragma unroll
    for (int r = 0; r < R; ++r)
      asm volatile("s_waitcnt lgkmcnt(%4)"
                   : "+v"(dst[r][0]), "+v"(dst[r][1]), "+v"(dst[r][2]), "+v"(acc[r])
                   : "n"(decltype(younger)::value)
                   : "memory");
  };
  int d[R];
#pragma unroll
  for (int r = 0; r < R; ++r) d[r] = dstp[r * GS * 16];
  read_step(0, a[0]);
#pragma unroll
  for (int r = 0; r < R; ++r) {
    d[r] = (int)__umul24((unsigned)d[r], (unsigned)acc_ld);
    old[r] = *reinterpret_cast<const f32x4 *>(accp + d[r]);
    acc[r] = f32x4{0.f, 0.f, 0.f, 0.f};
  }
  // (weight plane, row plane) by ascending magnitude: 2^-16 terms, 2^-8 terms, leading term
  constexpr int WP[6] = {2, 0, 1, 1, 0, 0};
  constexpr int AP[6] = {0, 2, 1, 0, 1, 0};
  auto step = [&](auto s_) {
    constexpr int S = decltype(s_)::value;
    if constexpr (S + 1 < KS) {
      read_step(S + 1, a[(S + 1) & 1]);
      // younger than the reads of step S: the reads of step S + 1 and, for S = 0, the R accumulator reads (the
      // counter has four bits: 15 over-waits by one read when R = 4)
      constexpr int kYounger = 3 * R + (S == 0 ? R : 0);
      wait_step(a[S & 1], acc, std::integral_constant<int, (kYounger > 15 ? 15 : kYounger)>{});
    } else {
      wait_step(a[S & 1], acc, std::integral_constant<int, (S == 0 ? R : 0)>{});
    }
#pragma unroll
    for (int t = 0; t < 6; ++t) {
#pragma unroll
      for (int r = 0; r < R; ++r)
        acc[r] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(w[WP[t]][S], a[S & 1][r][AP[t]], acc[r], 0, 0, 0);
    }
  };
  step(std::integral_constant<int, 0>{});
  if constexpr (KS > 1) step(std::integral_constant<int, 1>{});
  if constexpr (KS > 2) step(std::integral_constant<int, 2>{});
  if constexpr (KS > 3) step(std::integral_constant<int, 3>{});
  static_assert(KS <= 4, "KC <= 128");
#pragma unroll
  for (int r = 0; r < R; ++r) *reinterpret_cast<f32x4 *>(accp + d[r]) = old[r] + acc[r];
}

// phase cycle counters of the TIMED instrumentation build (debug variant 256; s_memtime ticks summed over wave 0 of
// every workgroup — a multiply-first wave): [0] barrier wait, [1] produce (split + stage write, incl. the wait for the
// gathered rows, + load issue), [4] multiply, [5] prologue, [6] epilogue; [7] = batches
__device__ unsigned long long d_x3_timing[8];

// Target-stationary tile kernel (plan, batches and epilogue as k_conv_tile_bf16 / k_conv_tile_f32).  Pipeline:
//   * two LDS stage buffers; batch b is multiplied from buffer b & 1 while batch b + 1 is split and written into the
//     other one: ONE barrier per batch;
//   * the waves of a workgroup are skewed ("ping-pong"): waves 0-3 multiply first and produce second, waves 4-7
//     produce first and multiply second.  Waves w and w + 4 sit on the same SIMD, so on every SIMD one wave feeds the
//     matrix pipe while the other issues the vector / LDS-store / load instructions of the next batch (the bf16 MFMA
//     co-issues with them, docs/HISTORY.md 3.1a);
//   * gathered rows are two batches ahead in registers (slot = batch parity), their indices three; a wave's weights
//     (its 16 columns, three planes) one batch ahead.  All loads are plain and unconditional so that hipcc's counted
//     s_waitcnt leaves the younger ones in flight.
// EXACT: c_src is a multiple of KC.  SMALL: 32-bit gather offsets (host-checked: < 2^24 rows, source < 4 GiB).
// c_src % 8 == 0 is required (a 32-byte piece is wholly inside the row or wholly beyond it).
template <int NC, int KC, bool EXACT, bool SMALL, bool TIMED = false>
__global__ __launch_bounds__(NC * 4 * x3_group_shares(NC), 1) void k_conv_tile_f32x3(
    const float *__restrict__ src, int c_src, const bf16x8 *__restrict__ wp, int c_dst,
    const int32_t *__restrict__ plan_src, const int32_t *__restrict__ plan_dst,
    const int32_t *__restrict__ batch_desc, const int32_t *__restrict__ tile_bptr,
    const int32_t *__restrict__ order, float *__restrict__ dst, int64_t n_tgt, int tile_rows, int batch_groups) {
  typedef int i32x2 __attribute__((ext_vector_type(2)));
  typedef StageLayout<KC> SL;
  constexpr int GS = x3_group_shares(NC);
  constexpr int CBW = NC / 16;         // column blocks (waves per group share)
  constexpr int WAVES = CBW * GS;
  constexpr int NT = WAVES * 64;
  constexpr int LD = SL::kLd;          // bf16 elements per staged row and plane
  constexpr int ACC_LD = NC + kAccPad;
  constexpr int KS = KC / 32;
  constexpr int F8 = KC / 8;           // 8-channel pieces per gathered row (32 bytes of fp32)
  constexpr int CAP = ME_MAX_BATCH_GROUPS * 16;
  constexpr int ITER = (CAP * F8 + NT - 1) / NT;
  constexpr int PLANE = CAP * LD;      // elements between the planes of a stage buffer
  static_assert(KC % 32 == 0, "KC must be a multiple of 32");
  static_assert(ME_MAX_BATCH_GROUPS == 4, "mma_groups runs cover at most 4 groups");
  (void)batch_groups;

  extern __shared__ __attribute__((aligned(16))) char smem[];
  float *s_acc = reinterpret_cast<float *>(smem);                              // [(tile_rows + 1) x ACC_LD]
  __bf16 *s_a = reinterpret_cast<__bf16 *>(s_acc + (tile_rows + 1) * ACC_LD);  // [2][3][64 x LD]
  int32_t *s_dst = reinterpret_cast<int32_t *>(s_a + 2 * 3 * PLANE);           // [2][64]

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int i16 = lane & 15;
  const int q = lane >> 4;
  const int tile = tile_bptr[gridDim.x + 1 + blockIdx.x];   // heaviest-first dispatch order (me_plan_build)
  const int col_base = blockIdx.y * NC;
  const int nchunks = (c_src + KC - 1) / KC;
  const int ncb = (c_dst + 15) / 16;
  const int wcb = wave % CBW;          // column block of this wave inside the slab
  const int share = wave / CBW;        // its groups of a batch: share, share + GS, ...
  const int cb = min(col_base / 16 + wcb, ncb - 1);
  const bool produce_first = wave >= 4;   // waves w and w + 4 share a SIMD: opposite phase order

  unsigned long long tm[7] = {0, 0, 0, 0, 0, 0, 0};
  unsigned long long t_prev = TIMED ? __builtin_amdgcn_s_memtime() : 0ull;
  auto tick = [&](int slot) {
    if (TIMED) {
      const unsigned long long now = __builtin_amdgcn_s_memtime();
      tm[slot] += now - t_prev;
      t_prev = now;
    }
  };
  for (int x = tid; x < (tile_rows + 1) * ACC_LD / 4; x += NT)
    reinterpret_cast<f32x4 *>(s_acc)[x] = f32x4{0.f, 0.f, 0.f, 0.f};
  constexpr int ORD = (ME_MAX_TILE_ROWS + NT - 1) / NT;
  int32_t my_ord[ORD];
#pragma unroll
  for (int j = 0; j < ORD; ++j) {
    const int r = j * NT + tid;
    my_ord[j] = (order != nullptr && r < tile_rows && (int64_t)tile * tile_rows + r < n_tgt)
                    ? order[(int64_t)tile * tile_rows + r] : 0;
  }

  const int b0 = tile_bptr[tile];
  const int nb = tile_bptr[tile + 1] - b0;
  const int n_it = nb * nchunks;

  struct Desc {
    int chunk, g0, ng, k;
  };
  auto locate = [&](int it) {
    int r = min(it, n_it - 1);
    Desc d;
    d.chunk = 0;
    while (r >= nb) {
      r -= nb;
      ++d.chunk;
    }
    const i32x2 v = *reinterpret_cast<const i32x2 *>(batch_desc + 2 * (int64_t)(b0 + r));
    d.g0 = v.x;
    d.ng = v.y & 255;
    d.k = (int)((uint32_t)v.y >> 8);
    return d;
  };

  // registers of the batches in flight: slot = batch parity
  f32x4 stage[2][ITER][2];
  int32_t dstv[2] = {tile_rows, tile_rows};
  int32_t sidx[2][ITER];
  bf16x8 wreg[2][3][KS];

  // the 64-entry index window of a batch is read to its end unconditionally (the plan is followed by 64 valid
  // entries; threads beyond the window — wide workgroups on narrow chunks — re-read its last entry); padding slots
  // (index -1) gather row 0 and their products land in the dummy accumulator row
  auto load_sidx = [&](const Desc &d, int32_t (&sx)[ITER]) {
    const char *pb = reinterpret_cast<const char *>(plan_src + (int64_t)d.g0 * 16);
#pragma unroll
    for (int j = 0; j < ITER; ++j)
      sx[j] = *reinterpret_cast<const int32_t *>(pb + (unsigned)(min((j * NT + tid) / F8, CAP - 1) * 4));
  };
  const char *srcb = reinterpret_cast<const char *>(src);
  const unsigned row_bytes = (unsigned)c_src * 4u;
  auto gather = [&](const Desc &d, const int32_t (&sx)[ITER], f32x4 (&st)[ITER][2], int32_t &dv) {
    const int c0 = d.chunk * KC;
    dv = *reinterpret_cast<const int32_t *>(reinterpret_cast<const char *>(plan_dst + (int64_t)d.g0 * 16) +
                                           (unsigned)(min(tid, CAP - 1) * 4));
#pragma unroll
    for (int j = 0; j < ITER; ++j) {
      const int ch = c0 + ((j * NT + tid) % F8) * 8;
      const int chl = EXACT ? ch : min(ch, c_src - 8);
      const int sr = max(sx[j], 0);
      const f32x4 *p;
      if (SMALL) p = reinterpret_cast<const f32x4 *>(srcb + (__umul24((unsigned)sr, row_bytes) + (unsigned)chl * 4u));
      else p = reinterpret_cast<const f32x4 *>(src + (int64_t)sr * c_src + chl);
      st[j][0] = p[0];
      st[j][1] = p[1];
    }
  };
  auto write_stage = [&](const Desc &d, const f32x4 (&st)[ITER][2], int32_t dv, int buf) {
    const int c0 = d.chunk * KC;
    __bf16 *base = s_a + buf * 3 * PLANE;
    uint32_t flag = 0u;      // non-finite rows: conv_common.hpp (split3_flag / split3_fix)
#pragma unroll
    for (int j = 0; j < ITER; ++j) {
      const int idx = j * NT + tid;
      const int r = idx / F8;
      const int ch = c0 + (idx % F8) * 8;
      u32x4 p1, p2, p3;
      split3_raw(st[j][0], st[j][1], p1, p2, p3);
      flag = split3_flag(flag, p3);
      if (!EXACT && ch >= c_src) p1 = p2 = p3 = u32x4{0u, 0u, 0u, 0u};
      if (ITER * NT == CAP * F8 || r < CAP) {
        __bf16 *o = base + SL::off(r, idx % F8);
        *reinterpret_cast<u32x4 *>(o) = p1;
        *reinterpret_cast<u32x4 *>(o + PLANE) = p2;
        *reinterpret_cast<u32x4 *>(o + 2 * PLANE) = p3;
      }
    }
    if (__builtin_expect(__any(split3_suspect(flag)), 0)) {   // rare: split again, exactly, over the first attempt
#pragma unroll
      for (int j = 0; j < ITER; ++j) {
        const int idx = j * NT + tid;
        const int r = idx / F8;
        const int ch = c0 + (idx % F8) * 8;
        u32x4 p1, p2, p3;
        split3_fix(st[j][0], st[j][1], p1, p2, p3);
        if (!EXACT && ch >= c_src) p1 = p2 = p3 = u32x4{0u, 0u, 0u, 0u};
        if (ITER * NT == CAP * F8 || r < CAP) {
          __bf16 *o = base + SL::off(r, idx % F8);
          *reinterpret_cast<u32x4 *>(o) = p1;
          *reinterpret_cast<u32x4 *>(o + PLANE) = p2;
          *reinterpret_cast<u32x4 *>(o + 2 * PLANE) = p3;
        }
      }
    }
    if (tid < CAP) s_dst[buf * CAP + tid] = dv;
  };
  auto load_w = [&](const Desc &d, bf16x8 (&w)[3][KS]) {
    const bf16x8 *p = wp + (((((int64_t)d.k * nchunks + d.chunk) * ncb + cb) * 3) * KS) * 64 + lane;
#pragma unroll
    for (int pl = 0; pl < 3; ++pl) {
#pragma unroll
      for (int v = 0; v < KS; ++v) w[pl][v] = p[(pl * KS + v) * 64];
    }
  };
  // lane constants of the operand reads: row (share * 16 + i16) of the buffer, swizzled piece offsets per step
  int pofs[KS];
#pragma unroll
  for (int sx = 0; sx < KS; ++sx) pofs[sx] = ((sx * 4 + q) ^ SL::swz(i16)) * 8;
  auto multiply = [&](const Desc &d, const bf16x8 (&w)[3][KS], int buf) {
    const __bf16 *rowp = s_a + buf * 3 * PLANE + (share * 16 + i16) * LD;
    const int32_t *dstp = s_dst + buf * CAP + share * 16 + i16;
    float *accp = &s_acc[wcb * 16 + q * 4];
    const int mine = (d.ng - share + GS - 1) / GS;     // groups share, share + GS, ... below ng
    if constexpr (GS == 1 && KC < 96) {
      if (mine >= 4) mma_groups_f32x3<4, GS, KC>(rowp, pofs, w, dstp, accp, ACC_LD);
      else if (mine == 3) mma_groups_f32x3<3, GS, KC>(rowp, pofs, w, dstp, accp, ACC_LD);
    }
    if constexpr (GS == 1 && KC >= 96) {
      // three or four groups of a wide chunk in two runs: the operand registers of four groups x three steps,
      // two deep, do not fit next to the batches in flight
      if (mine >= 3) {
        mma_groups_f32x3<2, GS, KC>(rowp, pofs, w, dstp, accp, ACC_LD);
        if (mine >= 4) mma_groups_f32x3<2, GS, KC>(rowp + 32 * LD, pofs, w, dstp + 32, accp, ACC_LD);
        else mma_groups_f32x3<1, GS, KC>(rowp + 32 * LD, pofs, w, dstp + 32, accp, ACC_LD);
      }
    }
    if constexpr (GS <= 2) {
      if (mine == 2) mma_groups_f32x3<2, GS, KC>(rowp, pofs, w, dstp, accp, ACC_LD);
    }
    if (mine == 1) mma_groups_f32x3<1, GS, KC>(rowp, pofs, w, dstp, accp, ACC_LD);
  };

  if (n_it > 0) {
    // descriptors of batches it .. it + 4
    Desc dA = locate(0), dB = locate(1), dC = locate(2), dD = locate(3), dE = locate(4);
    // produce(x), x = the batch after the one being multiplied (slots NX = x & 1, CU = the other parity): split and
    // store its rows into buffer NX, request the indices of batch x + 3 and the rows of batch x + 2
    auto produce = [&](const Desc &dx, const Desc &dx2, const Desc &dx3, int buf, f32x4 (&st)[ITER][2], int32_t &dv,
                       int32_t (&sx_nx)[ITER], int32_t (&sx_cu)[ITER]) {
      write_stage(dx, st, dv, buf);
      load_sidx(dx3, sx_cu);          // batch x + 3: the slot held the indices of batch x + 1, already used
      gather(dx2, sx_nx, st, dv);     // batch x + 2 into the registers just stored
    };
    load_sidx(dA, sidx[0]);
    load_sidx(dB, sidx[1]);
    load_w(dA, wreg[0]);
    gather(dA, sidx[0], stage[0], dstv[0]);
    gather(dB, sidx[1], stage[1], dstv[1]);
    load_sidx(dC, sidx[0]);
    produce(dA, dC, dD, 0, stage[0], dstv[0], sidx[0], sidx[1]);   // batch 0 -> buffer 0
    tick(5);
    __syncthreads();

    // iteration `it` with parity P = it & 1: multiply batch it (buffer P, weights w_cu) and produce batch it + 1
    auto iteration = [&](int it, int P, bf16x8 (&w_cu)[3][KS], bf16x8 (&w_nx)[3][KS], f32x4 (&st_nx)[ITER][2],
                         int32_t &dv_nx, int32_t (&sx_nx)[ITER], int32_t (&sx_cu)[ITER]) {
      if (!produce_first) {
        load_w(dB, w_nx);
        multiply(dA, w_cu, P);
        if (TIMED) asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        tick(4);
        produce(dB, dD, dE, P ^ 1, st_nx, dv_nx, sx_nx, sx_cu);
        if (TIMED) asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        tick(1);
      } else {
        produce(dB, dD, dE, P ^ 1, st_nx, dv_nx, sx_nx, sx_cu);
        load_w(dB, w_nx);
        multiply(dA, w_cu, P);
      }
      __syncthreads();
      tick(0);
      dA = dB; dB = dC; dC = dD; dD = dE;
      dE = locate(it + 5);
    };
    int it = 0;
    for (; it + 1 < n_it; it += 2) {
      iteration(it, 0, wreg[0], wreg[1], stage[1], dstv[1], sidx[1], sidx[0]);
      iteration(it + 1, 1, wreg[1], wreg[0], stage[0], dstv[0], sidx[0], sidx[1]);
    }
    if (it < n_it) iteration(it, 0, wreg[0], wreg[1], stage[1], dstv[1], sidx[1], sidx[0]);
  } else {
    __syncthreads();
  }

  // every target row of the tile is written exactly once (rows without neighbours get zeros)
  const int64_t row0 = (int64_t)tile * tile_rows;
  const int rows_here = (int)min((int64_t)tile_rows, n_tgt - row0);
  const bool vec_out = (c_dst % 4) == 0;
  int32_t *s_ord = reinterpret_cast<int32_t *>(s_a);   // the stage buffers are free now
  if (order != nullptr) {
#pragma unroll
    for (int j = 0; j < ORD; ++j)
      if (j * NT + tid < tile_rows) s_ord[j * NT + tid] = my_ord[j];
    __syncthreads();
  }
  for (int x = tid; x < tile_rows * NC / 4; x += NT) {
    const int row = x / (NC / 4);
    const int c4 = x % (NC / 4);
    const int cc = col_base + c4 * 4;
    if (row < rows_here && cc < c_dst) {
      const f32x4 v = *reinterpret_cast<const f32x4 *>(&s_acc[row * ACC_LD + c4 * 4]);
      const int64_t grow = order ? (int64_t)s_ord[row] : row0 + row;
      float *o = dst + grow * c_dst + cc;
      if (vec_out) {
        *reinterpret_cast<f32x4 *>(o) = v;
      } else {
        o[0] = v.x;
        if (cc + 1 < c_dst) o[1] = v.y;
        if (cc + 2 < c_dst) o[2] = v.z;
        if (cc + 3 < c_dst) o[3] = v.w;
      }
    }
  }
  if (TIMED) {
    tick(6);
    if (tid == 0) {
#pragma unroll
      for (int t = 0; t < 7; ++t) atomicAdd(&d_x3_timing[t], tm[t]);
      atomicAdd(&d_x3_timing[7], (unsigned long long)n_it);
    }
  }
}

template <typename T>
__device__ __forceinline__ const T &only_arg(const T &t) { return t; }   // the one element of a parameter pack

// =================================================================================================
// wave-specialised variant (round 2, debug variant 31 until it is the default): k_conv_tile_f32x3_ws
// =================================================================================================
// Same plan, arithmetic, stage layout and epilogue as k_conv_tile_f32x3; what changes is who does what.  The
// ping-pong kernel gives every wave both jobs and 16 columns; its LDS budget per batch (operand reads 768 cycles —
// eight waves each read all 64 rows —, accumulator 740, stage writes 310) is above the 1536 MFMA cycles per SIMD it
// could run at.  Here waves 0-3 ONLY multiply, each NC / 4 columns (32 for a 128-column slab: every operand read
// feeds two column blocks, so the operand reads halve), and waves 4-7 ONLY produce (gather, split, stage); wave w
// and w + 4 share a SIMD, so every SIMD runs one matrix stream and one vector / memory stream, separated by the one
// barrier per batch.  A multiplier takes its groups in two passes of two (operand registers), operand reads one
// step ahead of the MFMAs (inline asm, see mma_groups_f32x3).
// NCW: multiplier waves.  4: NC / 4 columns each.  8 (128-column slabs, the default there): 16 columns each, two
// multipliers per SIMD next to the producer — the operand reads double again, but one multiplier's MFMAs cover the
// other's waits: forward 64 -> 128 11 - 17 % faster (scripts/check_variant.py).  (Eight multipliers on a 64-column slab,
// each taking one pass of a batch, were tried: KC = 128 no longer fits 168 registers, 64 -> 64 gains 3 %.)
// TAIL (the input-gradient launch of a layer whose weight gradient is the split kernel, me_conv_dgrad_reduce_tail_f32x3):
// the grid carries workgroups behind its tiles that do the REDUCE of that weight gradient (wgrad_reduce.hpp) instead
// of a tile — they are dispatched last, onto CUs that have run out of tiles, so the reduce needs no launch of its own.
// Stream order alone makes the partial images complete before this launch starts.  TAIL_ARG is then one WgTail (the
// reduce's arguments and the tile count, which gridDim.x no longer is); without TAIL the pack is empty and the kernel
// is, argument for argument and instruction for instruction, the one it was.
template <int NC, int KC, bool EXACT, bool SMALL, bool TIMED = false, int PRIO = 2, int ABL = 0, int NCW = 4,
          bool TAIL = false, typename... TAIL_ARG>
__global__ __launch_bounds__((NCW + 4) * 64, 1) void k_conv_tile_f32x3_ws(
    const float *__restrict__ src, int c_src, const bf16x8 *__restrict__ wp, int c_dst,
    const int32_t *__restrict__ plan_src, const int32_t *__restrict__ plan_dst,
    const int32_t *__restrict__ batch_desc, const int32_t *__restrict__ tile_bptr,
    const int32_t *__restrict__ order, float *__restrict__ dst, int64_t n_tgt, int tile_rows, int batch_groups,
    TAIL_ARG... tail) {
  static_assert(sizeof...(TAIL_ARG) == (TAIL ? 1 : 0), "TAIL: exactly one WgTail argument");
  typedef int i32x2 __attribute__((ext_vector_type(2)));
  typedef StageLayout<KC> SL;
  static_assert(NC == 64 || NC == 128, "multiplier waves of 16 or 32 columns");
  static_assert(NCW == 4 || (NCW == 8 && NC == 128), "four multiplier waves, or eight on a 128-column slab");
  constexpr int CB = NC / (16 * NCW);  // 16-column blocks per multiplier wave
  constexpr int NTP = 256;             // producer threads (four waves)
  constexpr int NT = NCW * 64 + NTP;   // threads
  constexpr int LD = SL::kLd;
  constexpr int ACC_LD = NC + kAccPad;
  constexpr int KS = KC / 32;
  constexpr int F8 = KC / 8;
  constexpr int CAP = ME_MAX_BATCH_GROUPS * 16;
  constexpr int ITER = (CAP * F8 + NTP - 1) / NTP;
  constexpr int PLANE = CAP * LD;
  (void)batch_groups;

  extern __shared__ __attribute__((aligned(16))) char smem[];
  unsigned n_tiles = gridDim.x;
  if constexpr (TAIL) {
    // the workgroups behind the tiles: the reduce (of the last slab row only), in the launch's LDS — they have no tile
    const WgTail &t = only_arg(tail...);
    n_tiles = (unsigned)t.n_tiles;
    if (blockIdx.x >= n_tiles) {
      if (blockIdx.y + 1 == gridDim.y) wgrad_reduce_tail<NT>(t.r, t.nb, (int)(blockIdx.x - n_tiles), smem);
      return;
    }
  }
  float *s_acc = reinterpret_cast<float *>(smem);                              // [(tile_rows + 1) x ACC_LD]
  __bf16 *s_a = reinterpret_cast<__bf16 *>(s_acc + (tile_rows + 1) * ACC_LD);  // [2][3][64 x LD]
  int32_t *s_dst = reinterpret_cast<int32_t *>(s_a + 2 * 3 * PLANE);           // [2][64]

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int i16 = lane & 15;
  const int q = lane >> 4;
  const int tile = tile_bptr[n_tiles + 1 + blockIdx.x];   // heaviest-first dispatch order (me_plan_build)
  const int col_base = blockIdx.y * NC;
  const int nchunks = (c_src + KC - 1) / KC;
  const int ncb = (c_dst + 15) / 16;

  for (int x = tid; x < (tile_rows + 1) * ACC_LD / 4; x += NT)
    reinterpret_cast<f32x4 *>(s_acc)[x] = f32x4{0.f, 0.f, 0.f, 0.f};
  constexpr int ORD = (ME_MAX_TILE_ROWS + NT - 1) / NT;
  int32_t my_ord[ORD];
#pragma unroll
  for (int j = 0; j < ORD; ++j) {
    const int r = j * NT + tid;
    my_ord[j] = (order != nullptr && r < tile_rows && (int64_t)tile * tile_rows + r < n_tgt)
                    ? order[(int64_t)tile * tile_rows + r] : 0;
  }

  const int b0 = tile_bptr[tile];
  const int nb = tile_bptr[tile + 1] - b0;
  const int n_it = nb * nchunks;
  struct Desc {
    int chunk, g0, ng, k;
  };
  auto locate = [&](int it) {
    int r = min(it, n_it - 1);
    Desc d;
    d.chunk = 0;
    while (r >= nb) {
      r -= nb;
      ++d.chunk;
    }
    const i32x2 v = *reinterpret_cast<const i32x2 *>(batch_desc + 2 * (int64_t)(b0 + r));
    d.g0 = v.x;
    d.ng = v.y & 255;
    d.k = (int)((uint32_t)v.y >> 8);
    return d;
  };

  if (n_it > 0 && wave >= NCW) {
    // ------------------------------------------------ producer waves ------------------------------------------------
    const int ptid = tid - NCW * 64;
    f32x4 stage[2][ITER][2];
    int32_t dstv[2] = {tile_rows, tile_rows};
    int32_t sidx[2][ITER];
    auto load_sidx = [&](const Desc &d, int32_t (&sx)[ITER]) {
      const char *pb = reinterpret_cast<const char *>(plan_src + (int64_t)d.g0 * 16);
#pragma unroll
      for (int j = 0; j < ITER; ++j)
        sx[j] = *reinterpret_cast<const int32_t *>(pb + (unsigned)(min((j * NTP + ptid) / F8, CAP - 1) * 4));
    };
    const char *srcb = reinterpret_cast<const char *>(src);
    const unsigned row_bytes = (unsigned)c_src * 4u;
    auto gather = [&](const Desc &d, const int32_t (&sx)[ITER], f32x4 (&st)[ITER][2], int32_t &dv) {
      const int c0 = d.chunk * KC;
      dv = *reinterpret_cast<const int32_t *>(reinterpret_cast<const char *>(plan_dst + (int64_t)d.g0 * 16) +
                                             (unsigned)(min(ptid, CAP - 1) * 4));
#pragma unroll
      for (int j = 0; j < ITER; ++j) {
        const int ch = c0 + ((j * NTP + ptid) % F8) * 8;
        const int chl = EXACT ? ch : min(ch, c_src - 8);
        const int sr = max(sx[j], 0);
        const f32x4 *p;
        if (SMALL) p = reinterpret_cast<const f32x4 *>(srcb + (__umul24((unsigned)sr, row_bytes) + (unsigned)chl * 4u));
        else p = reinterpret_cast<const f32x4 *>(src + (int64_t)sr * c_src + chl);
        st[j][0] = p[0];
        st[j][1] = p[1];
      }
    };
    auto write_stage = [&](const Desc &d, const f32x4 (&st)[ITER][2], int32_t dv, int buf) {
      const int c0 = d.chunk * KC;
      __bf16 *base = s_a + buf * 3 * PLANE;
      uint32_t flag = 0u;      // non-finite rows: conv_common.hpp (split3_flag / split3_fix)
#pragma unroll
      for (int j = 0; j < ITER; ++j) {
        const int idx = j * NTP + ptid;
        const int r = idx / F8;
        const int ch = c0 + (idx % F8) * 8;
        u32x4 p1, p2, p3;
        split3_raw(st[j][0], st[j][1], p1, p2, p3);
        flag = split3_flag(flag, p3);
        if (!EXACT && ch >= c_src) p1 = p2 = p3 = u32x4{0u, 0u, 0u, 0u};
        if (ITER * NTP == CAP * F8 || r < CAP) {
          __bf16 *o = base + SL::off(r, idx % F8);
          *reinterpret_cast<u32x4 *>(o) = p1;
          *reinterpret_cast<u32x4 *>(o + PLANE) = p2;
          *reinterpret_cast<u32x4 *>(o + 2 * PLANE) = p3;
        }
      }
      if (__builtin_expect(__any(split3_suspect(flag)), 0)) {   // rare: split again, exactly, over the first attempt
#pragma unroll
        for (int j = 0; j < ITER; ++j) {
          const int idx = j * NTP + ptid;
          const int r = idx / F8;
          const int ch = c0 + (idx % F8) * 8;
          u32x4 p1, p2, p3;
          split3_fix(st[j][0], st[j][1], p1, p2, p3);
          if (!EXACT && ch >= c_src) p1 = p2 = p3 = u32x4{0u, 0u, 0u, 0u};
          if (ITER * NTP == CAP * F8 || r < CAP) {
            __bf16 *o = base + SL::off(r, idx % F8);
            *reinterpret_cast<u32x4 *>(o) = p1;
            *reinterpret_cast<u32x4 *>(o + PLANE) = p2;
            *reinterpret_cast<u32x4 *>(o + 2 * PLANE) = p3;
          }
        }
      }
      if (ptid < CAP) s_dst[buf * CAP + ptid] = dv;
    };
    // produce(x): store batch x into buffer x & 1, request the indices of batch x + 3 and the rows of batch x + 2
    bool started = false;
    auto produce = [&](const Desc &dx, const Desc &dx2, const Desc &dx3, int buf, f32x4 (&st)[ITER][2], int32_t &dv,
                       int32_t (&sx_nx)[ITER], int32_t (&sx_cu)[ITER]) {
      if (ABL != 6) write_stage(dx, st, dv, buf);      // (ABL 6: no split / stage stores; 5: no gathers after the first)
      load_sidx(dx3, sx_cu);
      if (ABL != 5 || !started) gather(dx2, sx_nx, st, dv);
    };
    Desc dA = locate(0), dB = locate(1), dC = locate(2), dD = locate(3), dE = locate(4);
    load_sidx(dA, sidx[0]);
    load_sidx(dB, sidx[1]);
    gather(dA, sidx[0], stage[0], dstv[0]);
    gather(dB, sidx[1], stage[1], dstv[1]);
    load_sidx(dC, sidx[0]);
    produce(dA, dC, dD, 0, stage[0], dstv[0], sidx[0], sidx[1]);   // batch 0 -> buffer 0
    started = true;
    __syncthreads();
    unsigned long long tm_a = 0, tm_b = 0, t_prev = TIMED ? __builtin_amdgcn_s_memtime() : 0ull;
    auto iteration = [&](int it, int P, f32x4 (&st_nx)[ITER][2], int32_t &dv_nx, int32_t (&sx_nx)[ITER],
                         int32_t (&sx_cu)[ITER]) {
      produce(dB, dD, dE, P ^ 1, st_nx, dv_nx, sx_nx, sx_cu);   // batch it + 1 while batch it is multiplied
      if (TIMED) {
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        const unsigned long long now = __builtin_amdgcn_s_memtime();
        tm_a += now - t_prev;
        t_prev = now;
      }
      __syncthreads();
      if (TIMED) {
        const unsigned long long now = __builtin_amdgcn_s_memtime();
        tm_b += now - t_prev;
        t_prev = now;
      }
      dA = dB; dB = dC; dC = dD; dD = dE;
      dE = locate(it + 5);
    };
    int it = 0;
    for (; it + 1 < n_it; it += 2) {
      iteration(it, 0, stage[1], dstv[1], sidx[1], sidx[0]);
      iteration(it + 1, 1, stage[0], dstv[0], sidx[0], sidx[1]);
    }
    if (it < n_it) iteration(it, 0, stage[1], dstv[1], sidx[1], sidx[0]);
    if (TIMED && tid == NCW * 64) {
      atomicAdd(&d_x3_timing[1], tm_a);   // producer: split + stage write + load issue
      atomicAdd(&d_x3_timing[2], tm_b);   // producer: barrier wait
    }
  } else if (n_it > 0) {
    // ----------------------------------------------- multiplier waves -----------------------------------------------
    // (the matrix stream wins the issue arbitration against the producer wave of its SIMD)
    __builtin_amdgcn_s_setprio(PRIO);
    const int cbi0 = col_base / 16 + wave * CB;
    bf16x8 w[2][CB][3][KS];
    auto load_w = [&](const Desc &d, bf16x8 (&wd)[CB][3][KS]) {
#pragma unroll
      for (int c = 0; c < CB; ++c) {
        const bf16x8 *p = wp + (((((int64_t)d.k * nchunks + d.chunk) * ncb + min(cbi0 + c, ncb - 1)) * 3) * KS) * 64 + lane;
#pragma unroll
        for (int pl = 0; pl < 3; ++pl) {
#pragma unroll
          for (int v = 0; v < KS; ++v) wd[c][pl][v] = p[(pl * KS + v) * 64];
        }
      }
    };
    int pofs[KS];
#pragma unroll
    for (int sx = 0; sx < KS; ++sx) pofs[sx] = ((sx * 4 + q) ^ SL::swz(i16)) * 8;
    auto multiply = [&](const Desc &d, const bf16x8 (&wc)[CB][3][KS], int buf, auto &&next_w) {
      const __bf16 *rowp = s_a + buf * 3 * PLANE + i16 * LD;
      const int32_t *dstp = s_dst + buf * CAP + i16;
      float *accp = &s_acc[wave * CB * 16 + q * 4];
      // groups 0, 1 then 2, 3 (two passes keep the operand registers of a pass at 2 x 3 planes, two steps deep)
      if (d.ng >= 4) consume_batch_ws<2, 2, CB, KC, 3, ABL>(rowp, pofs, wc, dstp, accp, ACC_LD, next_w);
      else if (d.ng == 3) consume_batch_ws<2, 1, CB, KC, 3, ABL>(rowp, pofs, wc, dstp, accp, ACC_LD, next_w);
      else if (d.ng == 2) consume_batch_ws<2, 0, CB, KC, 3, ABL>(rowp, pofs, wc, dstp, accp, ACC_LD, next_w);
      else consume_batch_ws<1, 0, CB, KC, 3, ABL>(rowp, pofs, wc, dstp, accp, ACC_LD, next_w);
    };
    Desc dA = locate(0), dB = locate(1);
    load_w(dA, w[0]);
    __syncthreads();                      // batch 0 is staged
    unsigned long long tm_a = 0, tm_b = 0, t_prev = TIMED ? __builtin_amdgcn_s_memtime() : 0ull;
    auto iteration = [&](int it, int P, bf16x8 (&w_cu)[CB][3][KS], bf16x8 (&w_nx)[CB][3][KS]) {
      multiply(dA, w_cu, P, [&]() {
        if (ABL != 4 || it == 0) load_w(dB, w_nx);    // (ABL 4: the weights are loaded once — timing ablation)
      });
      if (TIMED) {
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        const unsigned long long now = __builtin_amdgcn_s_memtime();
        tm_a += now - t_prev;
        t_prev = now;
      }
      __syncthreads();
      if (TIMED) {
        const unsigned long long now = __builtin_amdgcn_s_memtime();
        tm_b += now - t_prev;
        t_prev = now;
      }
      dA = dB;
      dB = locate(it + 2);
    };
    int it = 0;
    for (; it + 1 < n_it; it += 2) {
      iteration(it, 0, w[0], w[1]);
      iteration(it + 1, 1, w[1], w[0]);
    }
    if (it < n_it) iteration(it, 0, w[0], w[1]);
    if (TIMED && tid == 0) {
      atomicAdd(&d_x3_timing[4], tm_a);   // multiplier: weights issue + multiply
      atomicAdd(&d_x3_timing[0], tm_b);   // multiplier: barrier wait
      atomicAdd(&d_x3_timing[7], (unsigned long long)n_it);
    }
  } else {
    __syncthreads();
  }

  // every target row of the tile is written exactly once (rows without neighbours get zeros)
  const int64_t row0 = (int64_t)tile * tile_rows;
  const int rows_here = (int)min((int64_t)tile_rows, n_tgt - row0);
  const bool vec_out = (c_dst % 4) == 0;
  int32_t *s_ord = reinterpret_cast<int32_t *>(s_a);   // the stage buffers are free now
  if (order != nullptr) {
#pragma unroll
    for (int j = 0; j < ORD; ++j)
      if (j * NT + tid < tile_rows) s_ord[j * NT + tid] = my_ord[j];
    __syncthreads();
  }
  for (int x = tid; x < tile_rows * NC / 4; x += NT) {
    const int row = x / (NC / 4);
    const int c4 = x % (NC / 4);
    const int cc = col_base + c4 * 4;
    if (row < rows_here && cc < c_dst) {
      const f32x4 v = *reinterpret_cast<const f32x4 *>(&s_acc[row * ACC_LD + c4 * 4]);
      const int64_t grow = order ? (int64_t)s_ord[row] : row0 + row;
      float *o = dst + grow * c_dst + cc;
      if (vec_out) {
        *reinterpret_cast<f32x4 *>(o) = v;
      } else {
        o[0] = v.x;
        if (cc + 1 < c_dst) o[1] = v.y;
        if (cc + 2 < c_dst) o[2] = v.z;
        if (cc + 3 < c_dst) o[3] = v.w;
      }
    }
  }
}


#ifdef ME_DEBUG_VARIANTS   // (measured, not adopted: profiles/r06_ring_persistent_ab.md; tuning build only)
// =================================================================================================
// free-running variant (round 6): k_conv_tile_f32x3_ring
// =================================================================================================
// Same plan, arithmetic, stage layout, multiplier batch step (consume_batch_ws) and epilogue as
// k_conv_tile_f32x3_ws — outputs are bit-identical — but NO workgroup barrier inside the batch loop.  The barrier
// per batch phase-locks the waves: both multipliers of a SIMD wait for the LDS at the same time, run their MFMAs
// at the same time and store at the same time, and a batch costs max(produce, multiply) + the skew of twelve waves
// (matrix pipe busy 0.36, waves parked 0.35 by counter).  Here the stage buffers form a ring of NS slots with two
// LDS counters per slot: `full` (+1 per producer wave once its part of a batch is stored) and `free` (+1 per
// multiplier wave once it has read the batch).  A producer wave writes batch b into slot b % NS as soon as the
// NCW multipliers have released the slot's previous batch; a multiplier wave starts batch b as soon as the four
// producers have published it.  Multipliers own disjoint accumulator columns and never wait for each other, so the
// two of a SIMD drift apart and one's MFMAs cover the other's LDS round trips; producers run up to NS - 1 batches
// ahead.  LDS operations of one wave execute in order, so a counter update issued behind a wave's stage stores /
// operand reads is performed behind them.
// (inline asm on the LDS byte address: through a generic pointer the poll became a flat load with `s_waitcnt vmcnt(0)`,
// which drains the gathers and weight loads that are meant to stay in flight)
__device__ __forceinline__ unsigned ring_addr(const int32_t *p) {
  typedef __attribute__((address_space(3))) const char lds_char;
  return (unsigned)(uintptr_t)(lds_char *)p;
}
__device__ __forceinline__ void ring_wait(unsigned flag_addr, int target) {
  for (;;) {
    int v;
    asm volatile("ds_read_b32 %0, %1\n\ts_waitcnt lgkmcnt(0)" : "=v"(v) : "v"(flag_addr) : "memory");
    if (__builtin_amdgcn_readfirstlane(v) >= target) break;
    __builtin_amdgcn_s_sleep(1);
  }
}
__device__ __forceinline__ void ring_signal(unsigned flag_addr, int lane) {
  if (lane == 0) asm volatile("ds_add_u32 %0, %1" : : "v"(flag_addr), "v"(1) : "memory");
}

__host__ __device__ constexpr int conv_f32x3_ring_lds_bytes(int nc, int kc, int tile_rows, int ns) {
  return (tile_rows + 1) * (nc + kAccPad) * 4 + ns * ME_MAX_BATCH_GROUPS * 16 * (3 * x3_stage_ld(kc) * 2 + 4) + 64;
}

template <int NC, int KC, bool EXACT, bool SMALL, int NCW, int NS>
__global__ __launch_bounds__((NCW + 4) * 64, 1) void k_conv_tile_f32x3_ring(
    const float *__restrict__ src, int c_src, const bf16x8 *__restrict__ wp, int c_dst,
    const int32_t *__restrict__ plan_src, const int32_t *__restrict__ plan_dst,
    const int32_t *__restrict__ batch_desc, const int32_t *__restrict__ tile_bptr,
    const int32_t *__restrict__ order, float *__restrict__ dst, int64_t n_tgt, int tile_rows, int batch_groups) {
  typedef int i32x2 __attribute__((ext_vector_type(2)));
  typedef StageLayout<KC> SL;
  static_assert(NC == 64 || NC == 128, "multiplier waves of 16 or 32 columns");
  static_assert(NCW == 4 || (NCW == 8 && NC == 128), "four multiplier waves, or eight on a 128-column slab");
  static_assert(NS == 2 || NS == 3, "ring of two or three stage slots");
  constexpr int CB = NC / (16 * NCW);  // 16-column blocks per multiplier wave
  constexpr int NTP = 256;             // producer threads (four waves)
  constexpr int NT = NCW * 64 + NTP;   // threads
  constexpr int LD = SL::kLd;
  constexpr int ACC_LD = NC + kAccPad;
  constexpr int KS = KC / 32;
  constexpr int F8 = KC / 8;
  constexpr int CAP = ME_MAX_BATCH_GROUPS * 16;
  constexpr int ITER = (CAP * F8 + NTP - 1) / NTP;
  constexpr int PLANE = CAP * LD;
  (void)batch_groups;

  extern __shared__ __attribute__((aligned(16))) char smem[];
  float *s_acc = reinterpret_cast<float *>(smem);                              // [(tile_rows + 1) x ACC_LD]
  __bf16 *s_a = reinterpret_cast<__bf16 *>(s_acc + (tile_rows + 1) * ACC_LD);  // [NS][3][64 x LD]
  int32_t *s_dst = reinterpret_cast<int32_t *>(s_a + NS * 3 * PLANE);          // [NS][64]
  int32_t *s_full = s_dst + NS * CAP;                                          // [NS] producer waves that published
  int32_t *s_free = s_full + 4;                                                // [NS] multiplier waves that released
  const unsigned full_addr = ring_addr(s_full), free_addr = ring_addr(s_free);

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int i16 = lane & 15;
  const int q = lane >> 4;
  const int tile = tile_bptr[gridDim.x + 1 + blockIdx.x];   // heaviest-first dispatch order (me_plan_build)
  const int col_base = blockIdx.y * NC;
  const int nchunks = (c_src + KC - 1) / KC;
  const int ncb = (c_dst + 15) / 16;

  for (int x = tid; x < (tile_rows + 1) * ACC_LD / 4; x += NT)
    reinterpret_cast<f32x4 *>(s_acc)[x] = f32x4{0.f, 0.f, 0.f, 0.f};
  if (tid < 8) s_full[tid] = 0;
  constexpr int ORD = (ME_MAX_TILE_ROWS + NT - 1) / NT;
  int32_t my_ord[ORD];
#pragma unroll
  for (int j = 0; j < ORD; ++j) {
    const int r = j * NT + tid;
    my_ord[j] = (order != nullptr && r < tile_rows && (int64_t)tile * tile_rows + r < n_tgt)
                    ? order[(int64_t)tile * tile_rows + r] : 0;
  }

  const int b0 = tile_bptr[tile];
  const int nb = tile_bptr[tile + 1] - b0;
  const int n_it = nb * nchunks;
  struct Desc {
    int chunk, g0, ng, k;
  };
  auto locate = [&](int it) {
    int r = min(it, n_it - 1);
    Desc d;
    d.chunk = 0;
    while (r >= nb) {
      r -= nb;
      ++d.chunk;
    }
    const i32x2 v = *reinterpret_cast<const i32x2 *>(batch_desc + 2 * (int64_t)(b0 + r));
    d.g0 = v.x;
    d.ng = v.y & 255;
    d.k = (int)((uint32_t)v.y >> 8);
    return d;
  };

  if (n_it > 0 && wave >= NCW) {
    // ------------------------------------------------ producer waves ------------------------------------------------
    const int ptid = tid - NCW * 64;
    f32x4 stage[2][ITER][2];
    int32_t dstv[2] = {tile_rows, tile_rows};
    int32_t sidx[2][ITER];
    auto load_sidx = [&](const Desc &d, int32_t (&sx)[ITER]) {
      const char *pb = reinterpret_cast<const char *>(plan_src + (int64_t)d.g0 * 16);
#pragma unroll
      for (int j = 0; j < ITER; ++j)
        sx[j] = *reinterpret_cast<const int32_t *>(pb + (unsigned)(min((j * NTP + ptid) / F8, CAP - 1) * 4));
    };
    const char *srcb = reinterpret_cast<const char *>(src);
    const unsigned row_bytes = (unsigned)c_src * 4u;
    auto gather = [&](const Desc &d, const int32_t (&sx)[ITER], f32x4 (&st)[ITER][2], int32_t &dv) {
      const int c0 = d.chunk * KC;
      dv = *reinterpret_cast<const int32_t *>(reinterpret_cast<const char *>(plan_dst + (int64_t)d.g0 * 16) +
                                             (unsigned)(min(ptid, CAP - 1) * 4));
#pragma unroll
      for (int j = 0; j < ITER; ++j) {
        const int ch = c0 + ((j * NTP + ptid) % F8) * 8;
        const int chl = EXACT ? ch : min(ch, c_src - 8);
        const int sr = max(sx[j], 0);
        const f32x4 *p;
        if (SMALL) p = reinterpret_cast<const f32x4 *>(srcb + (__umul24((unsigned)sr, row_bytes) + (unsigned)chl * 4u));
        else p = reinterpret_cast<const f32x4 *>(src + (int64_t)sr * c_src + chl);
        st[j][0] = p[0];
        st[j][1] = p[1];
      }
    };
    auto write_stage = [&](const Desc &d, const f32x4 (&st)[ITER][2], int32_t dv, int slot) {
      const int c0 = d.chunk * KC;
      __bf16 *base = s_a + slot * 3 * PLANE;
      uint32_t flag = 0u;      // non-finite rows: conv_common.hpp (split3_flag / split3_fix)
#pragma unroll
      for (int j = 0; j < ITER; ++j) {
        const int idx = j * NTP + ptid;
        const int r = idx / F8;
        const int ch = c0 + (idx % F8) * 8;
        u32x4 p1, p2, p3;
        split3_raw(st[j][0], st[j][1], p1, p2, p3);
        flag = split3_flag(flag, p3);
        if (!EXACT && ch >= c_src) p1 = p2 = p3 = u32x4{0u, 0u, 0u, 0u};
        if (ITER * NTP == CAP * F8 || r < CAP) {
          __bf16 *o = base + SL::off(r, idx % F8);
          *reinterpret_cast<u32x4 *>(o) = p1;
          *reinterpret_cast<u32x4 *>(o + PLANE) = p2;
          *reinterpret_cast<u32x4 *>(o + 2 * PLANE) = p3;
        }
      }
      if (__builtin_expect(__any(split3_suspect(flag)), 0)) {   // rare: split again, exactly, over the first attempt
#pragma unroll
        for (int j = 0; j < ITER; ++j) {
          const int idx = j * NTP + ptid;
          const int r = idx / F8;
          const int ch = c0 + (idx % F8) * 8;
          u32x4 p1, p2, p3;
          split3_fix(st[j][0], st[j][1], p1, p2, p3);
          if (!EXACT && ch >= c_src) p1 = p2 = p3 = u32x4{0u, 0u, 0u, 0u};
          if (ITER * NTP == CAP * F8 || r < CAP) {
            __bf16 *o = base + SL::off(r, idx % F8);
            *reinterpret_cast<u32x4 *>(o) = p1;
            *reinterpret_cast<u32x4 *>(o + PLANE) = p2;
            *reinterpret_cast<u32x4 *>(o + 2 * PLANE) = p3;
          }
        }
      }
      if (ptid < CAP) s_dst[slot * CAP + ptid] = dv;
    };
    Desc dA = locate(0), dB = locate(1), dC = locate(2), dD = locate(3);
    load_sidx(dA, sidx[0]);
    load_sidx(dB, sidx[1]);
    gather(dA, sidx[0], stage[0], dstv[0]);
    gather(dB, sidx[1], stage[1], dstv[1]);
    load_sidx(dC, sidx[0]);
    __syncthreads();                      // accumulator tile and counters are zero
    int slot = 0, round = 0;
    // batch b: wait for its slot, split + store it, publish; then request the indices of batch b + 3 and the rows of
    // batch b + 2 (register slot = batch parity, as in k_conv_tile_f32x3_ws)
    auto iteration = [&](int b, f32x4 (&st)[ITER][2], int32_t &dv, int32_t (&sx_nx)[ITER], int32_t (&sx_cu)[ITER]) {
      if (round > 0) ring_wait(free_addr + 4u * slot, NCW * round);
      write_stage(dA, st, dv, slot);
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
      ring_signal(full_addr + 4u * slot, lane);
      load_sidx(dD, sx_cu);
      gather(dC, sx_nx, st, dv);
      dA = dB; dB = dC; dC = dD;
      dD = locate(b + 4);
      if (++slot == NS) {
        slot = 0;
        ++round;
      }
    };
    int b = 0;
    for (; b + 1 < n_it; b += 2) {
      iteration(b, stage[0], dstv[0], sidx[0], sidx[1]);
      iteration(b + 1, stage[1], dstv[1], sidx[1], sidx[0]);
    }
    if (b < n_it) iteration(b, stage[0], dstv[0], sidx[0], sidx[1]);
  } else if (n_it > 0) {
    // ----------------------------------------------- multiplier waves -----------------------------------------------
    __builtin_amdgcn_s_setprio(2);
    const int cbi0 = col_base / 16 + wave * CB;
    bf16x8 w[2][CB][3][KS];
    auto load_w = [&](const Desc &d, bf16x8 (&wd)[CB][3][KS]) {
#pragma unroll
      for (int c = 0; c < CB; ++c) {
        const bf16x8 *p = wp + (((((int64_t)d.k * nchunks + d.chunk) * ncb + min(cbi0 + c, ncb - 1)) * 3) * KS) * 64 + lane;
#pragma unroll
        for (int pl = 0; pl < 3; ++pl) {
#pragma unroll
          for (int v = 0; v < KS; ++v) wd[c][pl][v] = p[(pl * KS + v) * 64];
        }
      }
    };
    int pofs[KS];
#pragma unroll
    for (int sx = 0; sx < KS; ++sx) pofs[sx] = ((sx * 4 + q) ^ SL::swz(i16)) * 8;
    auto multiply = [&](const Desc &d, const bf16x8 (&wc)[CB][3][KS], int slot, auto &&next_w) {
      const __bf16 *rowp = s_a + slot * 3 * PLANE + i16 * LD;
      const int32_t *dstp = s_dst + slot * CAP + i16;
      float *accp = &s_acc[wave * CB * 16 + q * 4];
      if (d.ng >= 4) consume_batch_ws<2, 2, CB, KC, 3, 0>(rowp, pofs, wc, dstp, accp, ACC_LD, next_w);
      else if (d.ng == 3) consume_batch_ws<2, 1, CB, KC, 3, 0>(rowp, pofs, wc, dstp, accp, ACC_LD, next_w);
      else if (d.ng == 2) consume_batch_ws<2, 0, CB, KC, 3, 0>(rowp, pofs, wc, dstp, accp, ACC_LD, next_w);
      else consume_batch_ws<1, 0, CB, KC, 3, 0>(rowp, pofs, wc, dstp, accp, ACC_LD, next_w);
    };
    Desc dA = locate(0), dB = locate(1);
    load_w(dA, w[0]);
    __syncthreads();                      // accumulator tile and counters are zero
    int slot = 0, round = 0;
    auto iteration = [&](int b, bf16x8 (&w_cu)[CB][3][KS], bf16x8 (&w_nx)[CB][3][KS]) {
      ring_wait(full_addr + 4u * slot, 4 * (round + 1));
      multiply(dA, w_cu, slot, [&]() { load_w(dB, w_nx); });
      ring_signal(free_addr + 4u * slot, lane);
      dA = dB;
      dB = locate(b + 2);
      if (++slot == NS) {
        slot = 0;
        ++round;
      }
    };
    int b = 0;
    for (; b + 1 < n_it; b += 2) {
      iteration(b, w[0], w[1]);
      iteration(b + 1, w[1], w[0]);
    }
    if (b < n_it) iteration(b, w[0], w[1]);
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
  } else {
    __syncthreads();
  }
  __syncthreads();                        // every multiplier has added its last batch

  // every target row of the tile is written exactly once (rows without neighbours get zeros)
  const int64_t row0 = (int64_t)tile * tile_rows;
  const int rows_here = (int)min((int64_t)tile_rows, n_tgt - row0);
  const bool vec_out = (c_dst % 4) == 0;
  int32_t *s_ord = reinterpret_cast<int32_t *>(s_a);   // the stage buffers are free now
  if (order != nullptr) {
#pragma unroll
    for (int j = 0; j < ORD; ++j)
      if (j * NT + tid < tile_rows) s_ord[j * NT + tid] = my_ord[j];
    __syncthreads();
  }
  for (int x = tid; x < tile_rows * NC / 4; x += NT) {
    const int row = x / (NC / 4);
    const int c4 = x % (NC / 4);
    const int cc = col_base + c4 * 4;
    if (row < rows_here && cc < c_dst) {
      const f32x4 v = *reinterpret_cast<const f32x4 *>(&s_acc[row * ACC_LD + c4 * 4]);
      const int64_t grow = order ? (int64_t)s_ord[row] : row0 + row;
      float *o = dst + grow * c_dst + cc;
      if (vec_out) {
        *reinterpret_cast<f32x4 *>(o) = v;
      } else {
        o[0] = v.x;
        if (cc + 1 < c_dst) o[1] = v.y;
        if (cc + 2 < c_dst) o[2] = v.z;
        if (cc + 3 < c_dst) o[3] = v.w;
      }
    }
  }
}


// =================================================================================================
// persistent variant (round 6): k_conv_tile_f32x3_pers — tiles stream through ONE resident workgroup per CU
// =================================================================================================
// k_conv_tile_f32x3_ws holds one workgroup per CU (LDS), so every tile's prologue (zero fill, the dependent chain tile ->
// batch descriptors -> pair indices -> rows: three memory round trips) and epilogue (the accumulator tile to global
// memory, with every CU storing at the same moment) run with the matrix pipes idle: 5.8 of 27 us per tile by the phase
// counters (profiles/r04_ws_phase_timing.log).  Here a workgroup takes the tiles wg, wg + G, wg + 2 G, ... of the
// heaviest-first order (G = workgroups of the launch) as ONE stream of batches through the ring of
// k_conv_tile_f32x3_ring (two stage slots, full / free counters, no barrier), with TWO accumulator tiles: while the
// multipliers add tile s + 1 into one, the producer waves store tile s from the other (each wave its own rows, then
// zeros) as soon as the last multiplier has signalled it (`done`), and hand it back (`afree`) for tile s + 2.
// Only the producers walk the plan: a slot carries a header {groups, first / last / end flags, offset and chunk of the
// NEXT batch} from which a multiplier requests its weights one batch ahead.  Same plan, same sums in the same order:
// outputs are bit-identical to k_conv_tile_f32x3_ws.
// Every vector-memory load of the batch loop is unconditional (hipcc's counted `s_waitcnt vmcnt` keeps the younger
// gathers in flight only then; a first version with loads inside the tile roll-over ran at vmcnt(0): 2.2x slower): the
// workgroup's tiles {id, first batch, batches} sit in an LDS table filled before the loop, a row's output position is
// requested with every batch, the source-channel chunk of a batch is found without a loop (<= 4 chunks, host-checked).
constexpr int kPersMaxTiles = 192;   // tiles per workgroup the LDS table holds (host-checked)
constexpr int kPersMaxRows = 128;    // tallest tile
__host__ __device__ constexpr int conv_f32x3_pers_lds_bytes(int nc, int kc, int tile_rows) {
  return 2 * (tile_rows + 1) * (nc + kAccPad) * 4 + 2 * ME_MAX_BATCH_GROUPS * 16 * (3 * x3_stage_ld(kc) * 2 + 4) +
         3 * 16 + 64 + 2 * kPersMaxRows * 4 + kPersMaxTiles * 16;
}
__device__ __forceinline__ void lds_read4(unsigned addr, int &a, int &b, int &c, int &d) {
  typedef int i32x4_ __attribute__((ext_vector_type(4)));
  i32x4_ v;
  asm volatile("ds_read_b128 %0, %1\n\ts_waitcnt lgkmcnt(0)" : "=v"(v) : "v"(addr) : "memory");
  a = __builtin_amdgcn_readfirstlane(v.x);
  b = __builtin_amdgcn_readfirstlane(v.y);
  c = __builtin_amdgcn_readfirstlane(v.z);
  d = __builtin_amdgcn_readfirstlane(v.w);
}
__device__ __forceinline__ void lds_write4(unsigned addr, int a, int b, int c, int d) {
  typedef int i32x4_ __attribute__((ext_vector_type(4)));
  const i32x4_ v = {a, b, c, d};
  asm volatile("ds_write_b128 %0, %1" : : "v"(addr), "v"(v) : "memory");
}

template <int NC, int KC, int NCW>
__global__ __launch_bounds__((NCW + 4) * 64, 1) void k_conv_tile_f32x3_pers(
    const float *__restrict__ src, int c_src, const bf16x8 *__restrict__ wp, int c_dst,
    const int32_t *__restrict__ plan_src, const int32_t *__restrict__ plan_dst,
    const int32_t *__restrict__ batch_desc, const int32_t *__restrict__ tile_bptr,
    const int32_t *__restrict__ order, float *__restrict__ dst, int64_t n_tgt, int tile_rows, int n_tiles) {
  typedef int i32x2 __attribute__((ext_vector_type(2)));
  typedef __attribute__((address_space(3))) float lds_f32;
  typedef __attribute__((address_space(3))) int32_t lds_i32;
  typedef StageLayout<KC> SL;
  static_assert(NC == 64 || NC == 128, "multiplier waves of 16 or 32 columns");
  static_assert(NCW == 4 || (NCW == 8 && NC == 128), "four multiplier waves, or eight on a 128-column slab");
  constexpr int NS = 2;
  constexpr int CB = NC / (16 * NCW);  // 16-column blocks per multiplier wave
  constexpr int NTP = 256;             // producer threads (four waves)
  constexpr int NT = NCW * 64 + NTP;   // threads
  constexpr int LD = SL::kLd;
  constexpr int ACC_LD = NC + kAccPad;
  constexpr int KS = KC / 32;
  constexpr int F8 = KC / 8;
  constexpr int CAP = ME_MAX_BATCH_GROUPS * 16;
  constexpr int ITER = (CAP * F8 + NTP - 1) / NTP;
  constexpr int PLANE = CAP * LD;
  constexpr int EPN = ((kPersMaxRows / 4 + 1) * (NC / 4) + 63) / 64;   // 16-byte pieces of a tile per producer lane
  constexpr int F_FIRST = 1, F_LAST = 2, F_END = 4;

  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int acc_tile = (tile_rows + 1) * ACC_LD;                               // floats of one accumulator tile
  float *s_acc = reinterpret_cast<float *>(smem);                              // [2][(tile_rows + 1) x ACC_LD]
  __bf16 *s_a = reinterpret_cast<__bf16 *>(s_acc + 2 * acc_tile);              // [NS][3][64 x LD]
  int32_t *s_dst = reinterpret_cast<int32_t *>(s_a + NS * 3 * PLANE);          // [NS][64]
  int32_t *s_hdr = s_dst + NS * CAP;    // [NS + 1][4]: slot headers; [NS] = offset / chunk of the stream's first batch
  int32_t *s_flag = s_hdr + 3 * 4;      // [0..1] full, [4..5] free (stage slots); [8..9] done, [12..13] afree; [15] init
  int32_t *s_ord = s_flag + 16;         // [2][kPersMaxRows] output rows of an accumulator tile's rows
  int32_t *s_tiles = s_ord + 2 * kPersMaxRows;   // [kPersMaxTiles][4] this workgroup's tiles {id, first batch, batches}
  const unsigned full_addr = ring_addr(s_flag), free_addr = ring_addr(s_flag + 4);
  const unsigned done_addr = ring_addr(s_flag + 8), afree_addr = ring_addr(s_flag + 12), init_addr = ring_addr(s_flag + 15);
  const unsigned hdr_addr = ring_addr(s_hdr), tiles_addr = ring_addr(s_tiles);

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int i16 = lane & 15;
  const int q = lane >> 4;
  const int wg = blockIdx.x, G = gridDim.x;
  const int n_my = (n_tiles - wg + G - 1) / G;   // tiles of this workgroup (G <= n_tiles: at least one)
  const int col_base = blockIdx.y * NC;
  const int nchunks = c_src / KC;
  const int ncb = (c_dst + 15) / 16;

  for (int x = tid; x < 2 * acc_tile / 4; x += NT)
    reinterpret_cast<f32x4 *>(s_acc)[x] = f32x4{0.f, 0.f, 0.f, 0.f};
  if (tid < 16) s_flag[tid] = 0;
  for (int i = tid; i < n_my; i += NT) {
    const int tile = tile_bptr[n_tiles + 1 + wg + i * G];   // heaviest-first dispatch order (me_plan_build)
    const int b0 = tile_bptr[tile];
    s_tiles[4 * i + 0] = tile;
    s_tiles[4 * i + 1] = b0;
    s_tiles[4 * i + 2] = tile_bptr[tile + 1] - b0;
    s_tiles[4 * i + 3] = 0;
  }
  __syncthreads();                        // accumulator tiles, counters and the tile table are in place

  if (wave >= NCW) {
    // ------------------------------------------------ producer waves ------------------------------------------------
    const int ptid = tid - NCW * 64;
    const int pw = wave - NCW;
    struct Desc {
      int chunk, g0, ng, k;
      int seq, tile;          // running tile number of this workgroup (accumulator tile = seq & 1), tile id
      bool first, last, valid;
    };
    // the workgroup's batch stream: tiles in dispatch order, batches (x chunks) of a tile in plan order; past the end the
    // last batch again with valid = false (requested, never staged)
    int g_s = 0, g_it = 0, g_tile, g_b0, g_nb, g_nit;
    {
      int pad;
      lds_read4(tiles_addr, g_tile, g_b0, g_nb, pad);
      g_nit = max(g_nb * nchunks, 1);     // (a tile without pairs is one empty batch: its rows are written as zeros)
    }
    auto next = [&]() __attribute__((always_inline)) {
      if (g_it >= g_nit && g_s + 1 < n_my) {
        ++g_s;
        int pad;
        lds_read4(tiles_addr + 16u * g_s, g_tile, g_b0, g_nb, pad);
        g_nit = max(g_nb * nchunks, 1);
        g_it = 0;
      }
      Desc d;
      d.seq = g_s;
      d.tile = g_tile;
      d.valid = g_it < g_nit;
      const int it = min(g_it, g_nit - 1);
      d.first = it == 0;
      d.last = it == g_nit - 1;
      d.chunk = (it >= g_nb ? 1 : 0) + (it >= 2 * g_nb ? 1 : 0) + (it >= 3 * g_nb ? 1 : 0);
      d.g0 = 0;
      d.ng = 0;
      d.k = 0;
      if (g_nb > 0) {
        const i32x2 v = *reinterpret_cast<const i32x2 *>(batch_desc + 2 * (int64_t)(g_b0 + it - d.chunk * g_nb));
        d.g0 = v.x;
        d.ng = v.y & 255;
        d.k = (int)((uint32_t)v.y >> 8);
      } else {
        d.chunk = 0;
      }
      ++g_it;
      return d;
    };
    f32x4 stage[2][ITER][2];
    int32_t dstv[2] = {tile_rows, tile_rows};
    int32_t sidx[2][ITER];
    int32_t ordv[2];
    auto load_sidx = [&](const Desc &d, int32_t (&sx)[ITER]) {
      const char *pb = reinterpret_cast<const char *>(plan_src + (int64_t)d.g0 * 16);
#pragma unroll
      for (int j = 0; j < ITER; ++j)
        sx[j] = *reinterpret_cast<const int32_t *>(pb + (unsigned)(min((j * NTP + ptid) / F8, CAP - 1) * 4));
    };
    const char *srcb = reinterpret_cast<const char *>(src);
    const unsigned row_bytes = (unsigned)c_src * 4u;
    // lane l of producer wave pw requests the output row of tile row 4 l + pw (the wave stores the rows = pw mod 4)
    const int my_row = min(4 * (lane & 31) + pw, tile_rows - 1);
    auto gather = [&](const Desc &d, const int32_t (&sx)[ITER], f32x4 (&st)[ITER][2], int32_t &dv, int32_t &ov) {
      const int c0 = d.chunk * KC;
      dv = *reinterpret_cast<const int32_t *>(reinterpret_cast<const char *>(plan_dst + (int64_t)d.g0 * 16) +
                                             (unsigned)(min(ptid, CAP - 1) * 4));
      const int64_t orow = min((int64_t)d.tile * tile_rows + my_row, n_tgt - 1);
      ov = order != nullptr ? order[orow] : plan_dst[0];
      if (order == nullptr) ov = (int32_t)orow;
#pragma unroll
      for (int j = 0; j < ITER; ++j) {
        const int ch = c0 + ((j * NTP + ptid) % F8) * 8;
        const int sr = max(sx[j], 0);
        const f32x4 *p = reinterpret_cast<const f32x4 *>(srcb + (__umul24((unsigned)sr, row_bytes) + (unsigned)ch * 4u));
        st[j][0] = p[0];
        st[j][1] = p[1];
      }
    };
    auto write_stage = [&](const f32x4 (&st)[ITER][2], int32_t dv, int slot) {
      __bf16 *base = s_a + slot * 3 * PLANE;
      uint32_t flag = 0u;      // non-finite rows: conv_common.hpp (split3_flag / split3_fix)
#pragma unroll
      for (int j = 0; j < ITER; ++j) {
        const int idx = j * NTP + ptid;
        const int r = idx / F8;
        u32x4 p1, p2, p3;
        split3_raw(st[j][0], st[j][1], p1, p2, p3);
        flag = split3_flag(flag, p3);
        if (ITER * NTP == CAP * F8 || r < CAP) {
          __bf16 *o = base + SL::off(r, idx % F8);
          *reinterpret_cast<u32x4 *>(o) = p1;
          *reinterpret_cast<u32x4 *>(o + PLANE) = p2;
          *reinterpret_cast<u32x4 *>(o + 2 * PLANE) = p3;
        }
      }
      if (__builtin_expect(__any(split3_suspect(flag)), 0)) {   // rare: split again, exactly, over the first attempt
#pragma unroll
        for (int j = 0; j < ITER; ++j) {
          const int idx = j * NTP + ptid;
          const int r = idx / F8;
          u32x4 p1, p2, p3;
          split3_fix(st[j][0], st[j][1], p1, p2, p3);
          if (ITER * NTP == CAP * F8 || r < CAP) {
            __bf16 *o = base + SL::off(r, idx % F8);
            *reinterpret_cast<u32x4 *>(o) = p1;
            *reinterpret_cast<u32x4 *>(o + PLANE) = p2;
            *reinterpret_cast<u32x4 *>(o + 2 * PLANE) = p3;
          }
        }
      }
      if (ptid < CAP) s_dst[slot * CAP + ptid] = dv;
    };
    // the finished tile `ep_seq` (accumulator tile ep_seq & 1): this wave's rows (row = pw mod 4) to global memory, zeros
    // behind them
    int ep_seq = -1, ep_tile = 0;
    auto ep_ready = [&]() __attribute__((always_inline)) {
      int v;
      asm volatile("ds_read_b32 %0, %1\n\ts_waitcnt lgkmcnt(0)" : "=v"(v) : "v"(done_addr + 4u * (ep_seq & 1)) : "memory");
      return __builtin_amdgcn_readfirstlane(v) >= NCW * ((ep_seq >> 1) + 1);
    };
    auto ep_run = [&]() __attribute__((always_inline)) {
      lds_f32 *acc = (lds_f32 *)(s_acc + (ep_seq & 1) * acc_tile);
      const lds_i32 *ordl = (const lds_i32 *)(s_ord + (ep_seq & 1) * kPersMaxRows);
      const int64_t row0 = (int64_t)ep_tile * tile_rows;
      const int rows_here = (int)min((int64_t)tile_rows, n_tgt - row0);
      const bool vec_out = (c_dst % 4) == 0;
#pragma unroll 4
      for (int j = 0; j < EPN; ++j) {
        const int x = j * 64 + lane;
        const int row = 4 * (x / (NC / 4)) + pw;
        const int c4 = x % (NC / 4);
        const int cc = col_base + c4 * 4;
        if (row <= tile_rows) {
          typedef __attribute__((address_space(3))) f32x4 lds_f32x4;
          lds_f32x4 *a = (lds_f32x4 *)(acc + row * ACC_LD + c4 * 4);
          const f32x4 v = *a;
          *a = f32x4{0.f, 0.f, 0.f, 0.f};
          if (row < rows_here && cc < c_dst) {
            float *o = dst + (int64_t)ordl[row] * c_dst + cc;
            if (vec_out) {
              *reinterpret_cast<f32x4 *>(o) = v;
            } else {
              o[0] = v.x;
              if (cc + 1 < c_dst) o[1] = v.y;
              if (cc + 2 < c_dst) o[2] = v.z;
              if (cc + 3 < c_dst) o[3] = v.w;
            }
          }
        }
      }
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
      ring_signal(afree_addr + 4u * (ep_seq & 1), lane);
      ep_seq = -1;
    };
    Desc dA = next(), dB = next(), dC = next(), dD = next();
    load_sidx(dA, sidx[0]);
    load_sidx(dB, sidx[1]);
    gather(dA, sidx[0], stage[0], dstv[0], ordv[0]);
    gather(dB, sidx[1], stage[1], dstv[1], ordv[1]);
    load_sidx(dC, sidx[0]);
    if (ptid == 0) {
      lds_write4(hdr_addr + 16u * NS, dA.k, dA.chunk, 0, 0);
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
      ring_signal(init_addr, 0);
    }
    int slot = 0, round = 0;
    // batch b: wait for its slot, split + store it, publish it with its header; then request the indices of batch b + 3
    // and the rows of batch b + 2 (register slot = batch parity, as in k_conv_tile_f32x3_ws)
    auto iteration = [&](f32x4 (&st)[ITER][2], int32_t &dv, int32_t &ov, int32_t (&sx_nx)[ITER], int32_t (&sx_cu)[ITER]) {
      // the previous tile leaves as soon as the multipliers are through with it (at the latest NS batches into this
      // tile; before this tile's last batch in any case: its accumulator tile is the next one's)
      if (ep_seq >= 0) {
        bool go = true;
        if (dA.last) ring_wait(done_addr + 4u * (ep_seq & 1), NCW * ((ep_seq >> 1) + 1));
        else go = ep_ready();
        if (go) ep_run();
      }
      if (round > 0) ring_wait(free_addr + 4u * slot, NCW * round);
      if (dA.ng > 0) write_stage(st, dv, slot);
      if (ptid == 0)
        lds_write4(hdr_addr + 16u * slot, dA.ng, (dA.first ? F_FIRST : 0) | (dA.last ? F_LAST : 0) | (dB.valid ? 0 : F_END),
                   dB.k, dB.chunk);
      if (dA.last && lane < 32) ((lds_i32 *)s_ord)[(dA.seq & 1) * kPersMaxRows + min(4 * lane + pw, kPersMaxRows - 1)] = ov;
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
      ring_signal(full_addr + 4u * slot, lane);
      load_sidx(dD, sx_cu);
      gather(dC, sx_nx, st, dv, ov);
      if (dA.last) {
        ep_seq = dA.seq;
        ep_tile = dA.tile;
      }
      dA = dB; dB = dC; dC = dD;
      dD = next();
      if (++slot == NS) {
        slot = 0;
        ++round;
      }
    };
    for (;;) {
      if (!dA.valid) break;
      iteration(stage[0], dstv[0], ordv[0], sidx[0], sidx[1]);
      if (!dA.valid) break;
      iteration(stage[1], dstv[1], ordv[1], sidx[1], sidx[0]);
    }
    if (ep_seq >= 0) {
      ring_wait(done_addr + 4u * (ep_seq & 1), NCW * ((ep_seq >> 1) + 1));
      ep_run();
    }
  } else {
    // ----------------------------------------------- multiplier waves -----------------------------------------------
    __builtin_amdgcn_s_setprio(2);
    const int cbi0 = col_base / 16 + wave * CB;
    bf16x8 w[2][CB][3][KS];
    auto load_w = [&](int k, int chunk, bf16x8 (&wd)[CB][3][KS]) {
#pragma unroll
      for (int c = 0; c < CB; ++c) {
        const bf16x8 *p = wp + (((((int64_t)k * nchunks + chunk) * ncb + min(cbi0 + c, ncb - 1)) * 3) * KS) * 64 + lane;
#pragma unroll
        for (int pl = 0; pl < 3; ++pl) {
#pragma unroll
          for (int v = 0; v < KS; ++v) wd[c][pl][v] = p[(pl * KS + v) * 64];
        }
      }
    };
    int pofs[KS];
#pragma unroll
    for (int sx = 0; sx < KS; ++sx) pofs[sx] = ((sx * 4 + q) ^ SL::swz(i16)) * 8;
    auto multiply = [&](int ng, int buf, const bf16x8 (&wc)[CB][3][KS], int slot, auto &&next_w) {
      const __bf16 *rowp = s_a + slot * 3 * PLANE + i16 * LD;
      const int32_t *dstp = s_dst + slot * CAP + i16;
      float *accp = &s_acc[buf * acc_tile + wave * CB * 16 + q * 4];
      if (ng >= 4) consume_batch_ws<2, 2, CB, KC, 3, 0>(rowp, pofs, wc, dstp, accp, ACC_LD, next_w);
      else if (ng == 3) consume_batch_ws<2, 1, CB, KC, 3, 0>(rowp, pofs, wc, dstp, accp, ACC_LD, next_w);
      else if (ng == 2) consume_batch_ws<2, 0, CB, KC, 3, 0>(rowp, pofs, wc, dstp, accp, ACC_LD, next_w);
      else if (ng == 1) consume_batch_ws<1, 0, CB, KC, 3, 0>(rowp, pofs, wc, dstp, accp, ACC_LD, next_w);
      else next_w();
    };
    ring_wait(init_addr, 1);
    {
      int k0, chunk0, p0, p1;
      lds_read4(hdr_addr + 16u * NS, k0, chunk0, p0, p1);
      load_w(k0, chunk0, w[0]);
    }
    int slot = 0, round = 0, tile_n = 0;
    bool end = false;
    auto iteration = [&](bf16x8 (&w_cu)[CB][3][KS], bf16x8 (&w_nx)[CB][3][KS]) {
      ring_wait(full_addr + 4u * slot, 4 * (round + 1));
      int ng, fl, nk, nchunk;
      lds_read4(hdr_addr + 16u * slot, ng, fl, nk, nchunk);
      // the tile's accumulator: stored and zeroed by the producers after tile tile_n - 2
      if ((fl & F_FIRST) && tile_n >= 2) ring_wait(afree_addr + 4u * (tile_n & 1), 4 * (tile_n >> 1));
      multiply(ng, tile_n & 1, w_cu, slot, [&]() { load_w(nk, nchunk, w_nx); });
      ring_signal(free_addr + 4u * slot, lane);
      if (fl & F_LAST) {
        ring_signal(done_addr + 4u * (tile_n & 1), lane);   // (behind this wave's last stores: LDS order)
        ++tile_n;
      }
      end = (fl & F_END) != 0;
      if (++slot == NS) {
        slot = 0;
        ++round;
      }
    };
    for (;;) {
      iteration(w[0], w[1]);
      if (end) break;
      iteration(w[1], w[0]);
      if (end) break;
    }
  }
}

#endif  // ME_DEBUG_VARIANTS (ring / persistent kernels)

extern int g_conv_variant;  // conv.hip: variant 6 = 64-bit gather addresses, 256 = phase counters

struct ConvVariantX3 {
  int nc, slabs, kc;
};

static ConvVariantX3 conv_variant_f32x3(int c_src, int c_dst) {
  ConvVariantX3 v;
  // as many columns per workgroup as there are (up to 128, eight waves): the gather, the split and the stage writes
  // of a batch are paid once per workgroup, and with the cheap bf16 MFMAs they, not the matrix pipe, are the cost
  if (c_dst % 128 == 0) v.nc = 128;
  else if (c_dst % 96 == 0) v.nc = 96;
  else v.nc = c_dst <= 32 ? 32 : 64;
  v.slabs = (int)ceil_div(c_dst, v.nc);
  // widest chunk that tiles the source channels (one pass over the plan per chunk); 128 only next to <= 64 columns
  // (accumulator tile + three stage planes must fit the LDS)
  if (c_src % 128 == 0 && v.nc <= 64) v.kc = 128;
  else if (c_src % 64 == 0) v.kc = 64;
  else if (c_src % 96 == 0) v.kc = 96;
  else v.kc = c_src <= 32 ? 32 : 64;
  return v;
}

template <int NC, int KC>
static int launch_conv_tile_f32x3(const float *src, int c_src, const bf16x8 *wp, int c_dst, int slabs,
                                  const int32_t *plan_src, const int32_t *plan_dst, const int32_t *batch_desc,
                                  const int32_t *tile_bptr, const int32_t *order, float *dst, int64_t n_tgt,
                                  int tile_rows, int batch_groups, hipStream_t stream, bool small,
                                  const WgTail *tail = nullptr) {
  int lds = conv_f32x3_lds_bytes(NC, KC, tile_rows);
  ME_CHECK(lds <= kLdsBudget, "tile_rows too large for the LDS of one workgroup");
  const bool exact = (c_src % KC) == 0;
  // two instantiations per shape (round 6; four before): the fast one — source channels a multiple of the chunk AND 32-bit
  // gather offsets — and the general one, which also serves the two mixed cases (bit-identical results, a few per cent
  // slower on shapes no BASELINE configuration has)
  const bool fast = small && exact;
  typedef void (*kernel_t)(const float *, int, const bf16x8 *, int, const int32_t *, const int32_t *, const int32_t *,
                           const int32_t *, const int32_t *, float *, int64_t, int, int);
#ifdef ME_DEBUG_VARIANTS
  constexpr bool kHasPingPong = true;    // (tuning build: the round-2 ping-pong kernel for every shape, variants 30 / 256)
#else
  constexpr bool kHasPingPong = !(NC == 64 || NC == 128);   // shipped: only where no wave-specialised kernel exists
#endif
  kernel_t fn = nullptr;
  if constexpr (kHasPingPong)
    fn = fast ? &k_conv_tile_f32x3<NC, KC, true, true> : &k_conv_tile_f32x3<NC, KC, false, false>;
  if constexpr (NC == 64 || NC == 128) {
    // default: the wave-specialised kernel; debug variant 30 = the ping-pong kernel, 256 = its phase counters,
    // 257 = the wave-specialised kernel's phase counters (tuning build)
#ifdef ME_DEBUG_VARIANTS
    // free-running ring kernel (no barrier in the batch loop): exact 64- / 128-channel chunks with 32-bit offsets;
    // three stage slots where they fit next to the accumulator tile, else two.  Debug variant 40 selects it, 41 with two slots.
    if constexpr (KC == 64 || KC == 128) {
      if (small && exact && (g_conv_variant == 40 || g_conv_variant == 41)) {
        constexpr int RNCW = NC == 128 ? 8 : 4;
        constexpr bool kHas3 = KC == 64;
        const bool three = kHas3 && g_conv_variant != 41 && conv_f32x3_ring_lds_bytes(NC, KC, tile_rows, 3) <= kLdsBudget;
        kernel_t rk = &k_conv_tile_f32x3_ring<NC, KC, true, true, RNCW, 2>;
        if constexpr (kHas3) {
          if (three) rk = &k_conv_tile_f32x3_ring<NC, KC, true, true, RNCW, 3>;
        }
        const int rlds = conv_f32x3_ring_lds_bytes(NC, KC, tile_rows, three ? 3 : 2);
        ME_CHECK(rlds <= kLdsBudget, "tile_rows too large for the LDS of one workgroup (ring kernel)");
        static bool ring_attr[2] = {false, false};
        if (rlds > 48 * 1024 && !ring_attr[three ? 1 : 0]) {
          ME_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(rk), hipFuncAttributeMaxDynamicSharedMemorySize,
                                     kLdsBudget));
          ring_attr[three ? 1 : 0] = true;
        }
        const dim3 rgrid((unsigned)ceil_div(n_tgt, tile_rows), (unsigned)slabs);
        hipLaunchKernelGGL(rk, rgrid, dim3((RNCW + 4) * 64), (size_t)rlds, stream, src, c_src, wp, c_dst, plan_src, plan_dst,
                           batch_desc, tile_bptr, order, dst, n_tgt, tile_rows, batch_groups);
        ME_LAUNCH_CHECK();
        return 0;
      }
    }
    // persistent kernel (tiles stream through one resident workgroup per CU, two accumulator tiles): debug variant 43
    if constexpr (KC == 64 || KC == 128) {
      const int pers_tiles = (int)ceil_div(n_tgt, tile_rows);
      const int pers_wgs = std::min(pers_tiles, std::max(1, device_cu_count() / slabs));
      if (small && exact && g_conv_variant == 43 && tile_rows <= kPersMaxRows && c_src <= 4 * KC &&
          ceil_div(pers_tiles, pers_wgs) <= kPersMaxTiles && conv_f32x3_pers_lds_bytes(NC, KC, tile_rows) <= kLdsBudget) {
        constexpr int RNCW = NC == 128 ? 8 : 4;
        kernel_t pk = &k_conv_tile_f32x3_pers<NC, KC, RNCW>;
        const int plds = conv_f32x3_pers_lds_bytes(NC, KC, tile_rows);
        static bool pers_attr = false;
        if (plds > 48 * 1024 && !pers_attr) {
          ME_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(pk), hipFuncAttributeMaxDynamicSharedMemorySize,
                                     kLdsBudget));
          pers_attr = true;
        }
        const int n_tiles = pers_tiles, wgs = pers_wgs;
        hipLaunchKernelGGL(pk, dim3((unsigned)wgs, (unsigned)slabs), dim3((RNCW + 4) * 64), (size_t)plds, stream, src, c_src,
                           wp, c_dst, plan_src, plan_dst, batch_desc, tile_bptr, order, dst, n_tgt, tile_rows, n_tiles);
        ME_LAUNCH_CHECK();
        return 0;
      }
    }
#endif
    if (tail != nullptr) {
      // the wave-specialised kernel with the reduce of the layer's weight gradient behind its tiles (TAIL): the
      // same instantiation choice as below, n_tail more workgroups along grid.x
      typedef void (*tail_kernel_t)(const float *, int, const bf16x8 *, int, const int32_t *, const int32_t *,
                                    const int32_t *, const int32_t *, const int32_t *, float *, int64_t, int, int, WgTail);
      constexpr int TNCW = NC == 128 ? 8 : 4;
      constexpr int TNT = (TNCW + 4) * 64;
      const tail_kernel_t tk = fast ? &k_conv_tile_f32x3_ws<NC, KC, true, true, false, 2, 0, TNCW, true, WgTail>
                                    : &k_conv_tile_f32x3_ws<NC, KC, false, false, false, 2, 0, TNCW, true, WgTail>;
      const int tail_lds = (TNT / kWgReduceGroup) * kWgReduceGroupLds;
      if (lds < tail_lds) lds = tail_lds;
      static bool tail_attr[2] = {false, false};
      if (lds > 48 * 1024 && !tail_attr[fast ? 1 : 0]) {
        ME_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(tk), hipFuncAttributeMaxDynamicSharedMemorySize,
                                   kLdsBudget));
        tail_attr[fast ? 1 : 0] = true;
      }
      WgTail t = *tail;
      const int64_t n_tiles = ceil_div(n_tgt, tile_rows);
      const int64_t n_tail = ceil_div(wgrad_tail_groups(t), (int64_t)(TNT / kWgReduceGroup));
      ME_CHECK(n_tiles + n_tail < (1ll << 31), "grid too large");
      t.n_tiles = (int)n_tiles;
      hipLaunchKernelGGL(tk, dim3((unsigned)(n_tiles + n_tail), (unsigned)slabs), dim3(TNT), (size_t)lds, stream, src,
                         c_src, wp, c_dst, plan_src, plan_dst, batch_desc, tile_bptr, order, dst, n_tgt, tile_rows,
                         batch_groups, t);
      ME_LAUNCH_CHECK();
      return 0;
    }
    if (!kHasPingPong || (g_conv_variant != 30 && g_conv_variant != 256)) {
      kernel_t ws;
      int wi = (small ? 2 : 0) + (exact ? 1 : 0);
      int wthreads = 512;
      static bool ws_attr[20] = {};
      if constexpr (NC == 128) {
#ifdef ME_DEBUG_VARIANTS
        if (g_conv_variant == 31) {   // (tuning build: four multiplier waves)
          ws = fast ? &k_conv_tile_f32x3_ws<NC, KC, true, true> : &k_conv_tile_f32x3_ws<NC, KC, false, false>;
        } else
#endif
        {   // eight multiplier waves
          ws = fast ? &k_conv_tile_f32x3_ws<NC, KC, true, true, false, 2, 0, 8>
                    : &k_conv_tile_f32x3_ws<NC, KC, false, false, false, 2, 0, 8>;
          wi += 13;
          wthreads = 768;
        }
      } else {
        ws = fast ? &k_conv_tile_f32x3_ws<NC, KC, true, true> : &k_conv_tile_f32x3_ws<NC, KC, false, false>;
      }
#ifdef ME_DEBUG_VARIANTS   // phase counters, priority A/B and timing ablations (results invalid): tuning builds only
      if constexpr (KC >= 64) {
        if (g_conv_variant == 257 && small && exact) {
          ws = &k_conv_tile_f32x3_ws<NC, KC, true, true, true>;
          wi = 4;
          wthreads = 512;
        }
        if (g_conv_variant == 32 && small && exact) {   // A/B: no priority for the multiplier waves (four of them)
          ws = &k_conv_tile_f32x3_ws<NC, KC, true, true, false, 0>;
          wi = 5;
          wthreads = 512;
        }
        if (g_conv_variant >= 33 && g_conv_variant <= 38 && small && exact) {   // timing ablations (results invalid)
          ws = g_conv_variant == 33   ? &k_conv_tile_f32x3_ws<NC, KC, true, true, false, 2, 1>
               : g_conv_variant == 34 ? &k_conv_tile_f32x3_ws<NC, KC, true, true, false, 2, 2>
               : g_conv_variant == 35 ? &k_conv_tile_f32x3_ws<NC, KC, true, true, false, 2, 3>
               : g_conv_variant == 36 ? &k_conv_tile_f32x3_ws<NC, KC, true, true, false, 2, 4>
               : g_conv_variant == 37 ? &k_conv_tile_f32x3_ws<NC, KC, true, true, false, 2, 5>
                                      : &k_conv_tile_f32x3_ws<NC, KC, true, true, false, 2, 6>;
          wi = 3 + (g_conv_variant - 30);
          wthreads = 512;
        }
      }
#endif
      if (lds > 48 * 1024 && !ws_attr[wi]) {
        ME_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(ws), hipFuncAttributeMaxDynamicSharedMemorySize,
                                   kLdsBudget));
        ws_attr[wi] = true;
      }
      const dim3 wgrid((unsigned)ceil_div(n_tgt, tile_rows), (unsigned)slabs);
      hipLaunchKernelGGL(ws, wgrid, dim3(wthreads), (size_t)lds, stream, src, c_src, wp, c_dst, plan_src, plan_dst, batch_desc,
                         tile_bptr, order, dst, n_tgt, tile_rows, batch_groups);
      ME_LAUNCH_CHECK();
      return 0;
    }
  }
  bool timed = false;
#ifdef ME_DEBUG_VARIANTS
  constexpr bool kHasTimed = KC >= 64 && NC >= 64;   // instrumented build: the headline shapes only
  if constexpr (kHasTimed) {
    if (g_conv_variant == 256 && small && exact) {
      fn = &k_conv_tile_f32x3<NC, KC, true, true, true>;
      timed = true;
    }
  }
#endif
  static bool attr_set[5] = {false, false, false, false, false};  // per instantiation
  const int which = timed ? 4 : (small ? 2 : 0) + (exact ? 1 : 0);
  if (lds > 48 * 1024 && !attr_set[which]) {
    ME_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(fn), hipFuncAttributeMaxDynamicSharedMemorySize,
                               kLdsBudget));
    attr_set[which] = true;
  }
  const dim3 grid((unsigned)ceil_div(n_tgt, tile_rows), (unsigned)slabs);
  hipLaunchKernelGGL(fn, grid, dim3(NC * 4 * x3_group_shares(NC)), (size_t)lds, stream, src, c_src, wp, c_dst, plan_src, plan_dst, batch_desc,
                     tile_bptr, order, dst, n_tgt, tile_rows, batch_groups);
  ME_LAUNCH_CHECK();
  return 0;
}

}  // namespace me

using namespace me;

extern "C" {

int me_debug_conv_timing_f32x3(uint64_t *out8, int32_t reset) {
  unsigned long long h[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  if (out8 != nullptr) {
    ME_HIP(hipMemcpyFromSymbol(h, HIP_SYMBOL(d_x3_timing), sizeof(h)));
    for (int i = 0; i < 8; ++i) out8[i] = h[i];
  }
  if (reset) {
    unsigned long long z[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    ME_HIP(hipMemcpyToSymbol(HIP_SYMBOL(d_x3_timing), z, sizeof(z)));
  }
  return 0;
}

int32_t me_conv_f32x3_supported(int32_t c_src, int32_t c_dst) { return (c_src >= 8 && c_src % 8 == 0 && c_dst > 0) ? 1 : 0; }

int me_conv_plan_config_f32x3(int64_t n_tgt, int64_t volume, int64_t n_pairs, int32_t c_src, int32_t c_dst,
                              int32_t *tile_rows, int32_t *batch_groups) {
  ME_CHECK(tile_rows != nullptr && batch_groups != nullptr, "output pointers must not be null");
  *tile_rows = 128;
  *batch_groups = ME_MAX_BATCH_GROUPS;
  if (n_tgt <= 0 || volume <= 0 || c_src <= 0 || c_dst <= 0) return 0;
  const ConvVariantX3 v = conv_variant_f32x3(c_src, c_dst);
  PlanShape s;
  s.nc = v.nc;
  s.slabs = v.slabs;
  s.chunks = (int)ceil_div(c_src, v.kc);
  s.group_cycles = 32.0 + (v.kc / 32) * 96.0;   // six MFMAs per 32 channels + the accumulator round trip
  s.stage_row_bytes = 2 * (3 * x3_stage_ld(v.kc) * 2 + 4);   // two stage buffers
  s.max_occ = 1;   // eight waves per workgroup (six for 96 columns)
  *tile_rows = plan_tile_rows(s, n_tgt, volume, n_pairs);
  return 0;
}

int64_t me_conv_packed_weight_elems_f32x3(int64_t volume, int32_t c_src, int32_t c_dst) {   /* bf16 elements */
  if (volume <= 0 || c_src <= 0 || c_dst <= 0) return 0;
  const ConvVariantX3 v = conv_variant_f32x3(c_src, c_dst);
  return 3 * volume * align_up(c_src, v.kc) * align_up(c_dst, 16);
}

int32_t me_conv_pack_chunk_f32x3(int32_t c_src, int32_t c_dst) {
  return (c_src > 0 && c_dst > 0) ? conv_variant_f32x3(c_src, c_dst).kc : 0;
}

int me_conv_pack_weights_f32x3(const float *w, int64_t volume, int32_t c_src, int32_t c_dst, int32_t transposed,
                               uint16_t *wp, void *stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  ME_CHECK(volume >= 1 && c_src > 0 && c_dst > 0, "invalid weight shape");
  ME_CHECK((uintptr_t)wp % 16 == 0, "packed weights must be 16-byte aligned");
  const ConvVariantX3 v = conv_variant_f32x3(c_src, c_dst);
  const int nchunks = (int)ceil_div(c_src, v.kc), ncb = (int)ceil_div(c_dst, 16);
  const int64_t total = volume * nchunks * ncb * (v.kc / 32) * 64;  // threads: one 16-byte element per plane each
  u32x4 *wp4 = reinterpret_cast<u32x4 *>(wp);
  const dim3 grid((unsigned)ceil_div(total, 256)), block(256);
  if (v.kc == 128)
    hipLaunchKernelGGL((k_pack_weights_f32x3<128>), grid, block, 0, stream, w, c_src, c_dst, transposed, nchunks, ncb, wp4, total);
  else if (v.kc == 96)
    hipLaunchKernelGGL((k_pack_weights_f32x3<96>), grid, block, 0, stream, w, c_src, c_dst, transposed, nchunks, ncb, wp4, total);
  else if (v.kc == 64)
    hipLaunchKernelGGL((k_pack_weights_f32x3<64>), grid, block, 0, stream, w, c_src, c_dst, transposed, nchunks, ncb, wp4, total);
  else
    hipLaunchKernelGGL((k_pack_weights_f32x3<32>), grid, block, 0, stream, w, c_src, c_dst, transposed, nchunks, ncb, wp4, total);
  ME_LAUNCH_CHECK();
  return 0;
}

// me_conv_target_f32x3, and — tail != nullptr — the same launch with the weight-gradient reduce behind its tiles
static int conv_target_f32x3(const float *src, int64_t n_src, int32_t c_src, const uint16_t *wp_, int32_t c_dst,
                             const int32_t *plan_src, const int32_t *plan_dst, const int32_t *batch_desc,
                             const int32_t *tile_bptr, const int32_t *order, float *dst, int64_t n_tgt, int32_t tile_rows,
                             int32_t batch_groups, hipStream_t stream, const WgTail *tail) {
  ME_CHECK(me_conv_f32x3_supported(c_src, c_dst), "source channels must be a positive multiple of 8 (me_conv_f32x3_supported)");
  const bool small = n_src > 0 && n_src < (1ll << 24) && n_src * c_src * 4 < (1ll << 32) && g_conv_variant != 6;
  ME_CHECK(tile_rows >= ME_GROUP_ROWS && tile_rows <= ME_MAX_TILE_ROWS, "tile_rows out of range");
  ME_CHECK(batch_groups >= 1 && batch_groups <= ME_MAX_BATCH_GROUPS, "batch_groups out of range");
  ME_CHECK((uintptr_t)src % 16 == 0 && (uintptr_t)dst % 16 == 0 && (uintptr_t)wp_ % 16 == 0,
           "feature and weight pointers must be 16-byte aligned");
  if (n_tgt == 0) return 0;
  const bf16x8 *wp = reinterpret_cast<const bf16x8 *>(wp_);
  const ConvVariantX3 v = conv_variant_f32x3(c_src, c_dst);
  ME_CHECK(tail == nullptr || v.nc == 64 || v.nc == 128, "no reduce tail on this slab width (me_conv_dgrad_reduce_tail_supported)");
#define ME_CONV_CASE(NCV, KCV)                                                                                    \
  return launch_conv_tile_f32x3<NCV, KCV>(src, c_src, wp, c_dst, v.slabs, plan_src, plan_dst, batch_desc, tile_bptr, \
                                          order, dst, n_tgt, tile_rows, batch_groups, stream, small, tail)
  if (v.nc == 32) {
    if (v.kc == 128) ME_CONV_CASE(32, 128);
    if (v.kc == 96) ME_CONV_CASE(32, 96);
    if (v.kc == 64) ME_CONV_CASE(32, 64);
    ME_CONV_CASE(32, 32);
  } else if (v.nc == 64) {
    if (v.kc == 128) ME_CONV_CASE(64, 128);
    if (v.kc == 96) ME_CONV_CASE(64, 96);
    if (v.kc == 64) ME_CONV_CASE(64, 64);
    ME_CONV_CASE(64, 32);
  } else if (v.nc == 96) {
    if (v.kc == 96) ME_CONV_CASE(96, 96);
    if (v.kc == 64) ME_CONV_CASE(96, 64);
    ME_CONV_CASE(96, 32);
  } else {
    if (v.kc == 96) ME_CONV_CASE(128, 96);
    if (v.kc == 64) ME_CONV_CASE(128, 64);
    ME_CONV_CASE(128, 32);
  }
#undef ME_CONV_CASE
}

int me_conv_target_f32x3(const float *src, int64_t n_src, int32_t c_src, const uint16_t *wp_, int64_t volume,
                         int32_t c_dst, const int32_t *plan_src, const int32_t *plan_dst, const int32_t *batch_desc,
                         const int32_t *tile_bptr, const int32_t *order, float *dst, int64_t n_tgt, int32_t tile_rows,
                         int32_t batch_groups, void *stream_) {
  (void)volume;
  return conv_target_f32x3(src, n_src, c_src, wp_, c_dst, plan_src, plan_dst, batch_desc, tile_bptr, order, dst, n_tgt,
                           tile_rows, batch_groups, (hipStream_t)stream_, nullptr);
}

// ---- input gradient with the weight-gradient reduce as its tail ------------------------------------------------------
int g_dgrad_tail = 0;   // me_debug_set_dgrad_reduce_tail: 0 policy, 1 never (three launches), 2 wherever the kernels exist

// A tail workgroup fills a CU on its own (the launch's LDS), so the tail runs 8 - 12 waves per CU where k_wgrad_reduce
// runs 32: it pays while the tail is a few rounds of workgroups on CUs the tiles have left, not on wide layers whose
// reduce is many rounds long.  Measured per shape on the headline scene (scripts/dgrad_tail_sweep.py,
// profiles/r15_dgrad_reduce_tail_ab.md; tail workgroups, two-launch minus three-launch step): 64 -> 128 432, -8.5 us;
// 128 -> 64 288, -2.3; 128 -> 128 576, -9.1; 128 -> 256 1152, -10.4; 256 -> 128 1152 behind TWO slab rows of tiles,
// +5.2; 256 -> 256 2304, +27.4.  So: one slab row (c_in <= 128) and at most five rounds.
constexpr int kTailMaxRounds = 5;

int32_t me_conv_dgrad_reduce_tail_supported(int32_t c_in, int32_t c_out, int64_t volume, int64_t n_pairs) {
  if (g_dgrad_tail == 1 || volume < 1 || volume > 65535 || (g_conv_variant != 0 && g_conv_variant != 6)) return 0;
  if (!me_conv_f32x3_supported(c_out, c_in)) return 0;
  const ConvVariantX3 v = conv_variant_f32x3(c_out, c_in);   // the input gradient: source dy (c_out), target dx (c_in)
  if (v.nc != 64 && v.nc != 128) return 0;
  std::vector<int64_t> koffs((size_t)volume + 1, 0);   // (the geometry depends on the pair count alone)
  koffs[(size_t)volume] = n_pairs;
  WgTail t;
  if (!wgrad_split_tail(koffs.data(), nullptr, volume, c_in, c_out, nullptr, nullptr, &t)) return 0;
  if (g_dgrad_tail == 2) return 1;
  if (v.slabs != 1) return 0;
  const int groups_per_wg = v.nc == 128 ? 3 : 2;
  return ceil_div(wgrad_tail_groups(t), (int64_t)groups_per_wg) <= (int64_t)kTailMaxRounds * device_cu_count() ? 1 : 0;
}

void me_debug_set_dgrad_reduce_tail(int mode) { g_dgrad_tail = mode; }

int me_conv_dgrad_reduce_tail_f32x3(const float *dy, int64_t n_out, int32_t c_out, const uint16_t *wp_, int64_t volume,
                                    int32_t c_in, const int32_t *plan_src, const int32_t *plan_dst,
                                    const int32_t *batch_desc, const int32_t *tile_bptr, const int32_t *order, float *dx,
                                    int64_t n_in, int32_t tile_rows, int32_t batch_groups, const int64_t *k_offsets,
                                    const int64_t *k_offsets_dev, const void *workspace, int64_t workspace_bytes,
                                    float *grad_w, void *stream_) {
  ME_CHECK(n_in > 0, "no input rows: nothing carries the tail (me_conv_wgrad_f32 handles empty maps)");
  ME_CHECK(g_conv_variant == 0 || g_conv_variant == 6, "debug kernel variants have no reduce tail");
  ME_CHECK(k_offsets != nullptr && k_offsets_dev != nullptr && workspace != nullptr && grad_w != nullptr,
           "pair offsets, workspace and grad_w must not be null");
  ME_CHECK(workspace_bytes >= me_conv_wgrad_workspace_bytes(k_offsets, volume, c_in, c_out), "workspace too small");
  WgTail t;
  ME_CHECK(wgrad_split_tail(k_offsets, k_offsets_dev, volume, c_in, c_out, workspace, grad_w, &t),
           "not a split weight gradient (me_conv_dgrad_reduce_tail_supported)");
  return conv_target_f32x3(dy, n_out, c_out, wp_, c_in, plan_src, plan_dst, batch_desc, tile_bptr, order, dx, n_in,
                           tile_rows, batch_groups, (hipStream_t)stream_, &t);
}

}  // extern "C"

// code-object preload (me_preload, coords.hip): resolving one kernel of this translation unit makes the runtime load the
// unit's whole code object now instead of at the first launch from it
extern "C" __attribute__((visibility("hidden"))) void me_preload_conv_f32x3(void) {
  hipFuncAttributes attr;
  (void)hipFuncGetAttributes(&attr, reinterpret_cast<const void *>(&me::k_pack_weights_f32x3<128>));
}
