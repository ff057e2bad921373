// The second pass of the weight gradient: grad_w[k] = sum of the partial register images of the ranges that touch
// offset k.  One definition of the sums and their order, used by k_wgrad_reduce (conv.hip: a launch of its own) and by
// the reduce tail of the input-gradient launch (conv_f32x3.hip: k_conv_tile_f32x3_ws<..., TAIL = true>).
#pragma once
#include "conv_common.hpp"

namespace me {

constexpr int kWgMB = 4;  // 16-row MFMA blocks of input channels per wave (64 channels, one dwordx4 per lane)

__host__ __device__ __forceinline__ int64_t wgrad_range_begin(int64_t r, int64_t n_pairs, int64_t n_ranges) {
  return r * n_pairs / n_ranges;
}

// the range r with range_begin(r) <= e < range_begin(r + 1)
__device__ __forceinline__ int64_t wgrad_range_of_pair(int64_t e, int64_t n_pairs, int64_t n_ranges) {
  int64_t r = e * n_ranges / n_pairs;
  while (r > 0 && wgrad_range_begin(r, n_pairs, n_ranges) > e) --r;
  while (r + 1 < n_ranges && wgrad_range_begin(r + 1, n_pairs, n_ranges) <= e) ++r;
  return r;
}

constexpr int kWgReducePhases = 4;   // waves per group (16 measured slower: most offsets own ~10 slots, and 4x the
                                     // waves cost more than the long chain of the centre offset saves)
constexpr int kWgReduceGroup = 64 * kWgReducePhases;   // threads of a group: 256 consecutive floats of one image
// LDS of one group: its slot range (two int64, padded) and the phase sums
constexpr int kWgReduceGroupLds = 64 + kWgReducePhases * 64 * (int)sizeof(f32x4);

struct WgReduceArgs {
  const float *partial;    // [(ranges + volume) slots][n_cib][n_cob][image]
  const int64_t *koffs;    // device [volume + 1]
  float *grad_w;           // [volume][c_in][c_out]
  int64_t n_pairs;         // >= 1 (a map without pairs passes 1: every offset is empty)
  int volume, n_ranges, n_cib, n_cob, c_in, c_out;
};

// A GROUP of 256 threads (gtid & 255: 64 lanes x four phases) sums the 256 consecutive image floats [256 xb, 256 xb
// + 256) of offset k over the offset's slots and writes them to grad_w through the channel interleave of the kernel
// that made the images.  A thread owns FOUR consecutive floats (one 16-byte load per slot).  The waves take the slots
// first + phase, + PH, ... with eight independent loads in flight per thread (the centre offset of a sparse map owns
// half of all slots: its chain sets the duration, and the loop is latency-bound); the four phase sums are combined
// in phase order.  Per element: slots of a phase in ascending order, then the phases in order — a fixed order, so
// the result is bitwise reproducible and the same wherever this function runs.
// EVERY thread of the workgroup calls it (two barriers); `live` = false: a group without work.
// s_r / s_part: the group's kWgReduceGroupLds bytes of LDS.
// TR: the images come from the LDS-staged kernels (MFMA row i of block m <-> input channel 16*m + i, column j of
// block n <-> output channel 16*n + j) instead of k_wgrad_f32's interleave.
template <int NB, bool TR, int MB>
__device__ __forceinline__ void wgrad_reduce_group(const WgReduceArgs &a, int k, int xb, int gtid, bool live,
                                                   int64_t *s_r, f32x4 *s_part) {
  static_assert(MB == 4 || MB == 8, "input-channel blocks per workgroup");
  constexpr int kImage = MB * NB * 4 * 64;
  constexpr int PH = kWgReducePhases;
  const int n_cob = a.n_cob, c_in = a.c_in, c_out = a.c_out;
  if ((gtid & (kWgReduceGroup - 1)) == 0) {
    const int64_t b = a.koffs[k], e = a.koffs[k + 1];
    s_r[0] = 0;
    s_r[1] = -1;
    if (e > b) {
      s_r[0] = wgrad_range_of_pair(b, a.n_pairs, a.n_ranges) + k;
      s_r[1] = wgrad_range_of_pair(e - 1, a.n_pairs, a.n_ranges) + k;
    }
  }
  __syncthreads();
  const int j = gtid & 63, phase = (gtid >> 6) & (PH - 1);
  const int64_t idx = ((int64_t)xb * 64 + j) * 4;      // first of this thread's four floats (kImage % 256 == 0)
  const int64_t per_slot = (int64_t)a.n_cib * n_cob * kImage;
  live = live && idx < per_slot;
  f32x4 s = {0.f, 0.f, 0.f, 0.f};
  if (live) {
    const int64_t first = s_r[0], last = s_r[1];
    const float *p = a.partial + idx;
    int64_t slot = first + phase;
    for (; slot + 7 * PH <= last; slot += 8 * PH) {
      f32x4 v[8];
#pragma unroll
      for (int u = 0; u < 8; ++u) v[u] = *reinterpret_cast<const f32x4 *>(p + (slot + u * PH) * per_slot);
#pragma unroll
      for (int u = 0; u < 8; ++u) s += v[u];
    }
    for (; slot <= last; slot += PH) s += *reinterpret_cast<const f32x4 *>(p + slot * per_slot);
  }
  s_part[phase * 64 + j] = s;
  __syncthreads();
  if (phase != 0 || !live) return;
  s = s_part[j];
#pragma unroll
  for (int ph = 1; ph < PH; ++ph) s += s_part[ph * 64 + j];   // fixed order: bitwise reproducible
  // the four floats are four consecutive LANES of one register of the image (idx % 4 == 0, 64 lanes per register)
  const int lane0 = (int)(idx % 64);
  const int reg = (int)((idx / 64) % (MB * NB * 4));
  const int cob = (int)((idx / kImage) % n_cob);
  const int cib = (int)(idx / ((int64_t)kImage * n_cob));
  const int r = reg % 4, n = (reg / 4) % NB, m = reg / (4 * NB);
  const int q = lane0 >> 4;
  const int ci = cib * (16 * MB) + (TR ? 16 * m + 4 * q + r : MB * (4 * q + r) + m);
  if (ci >= c_in) return;
  float *row = a.grad_w + ((int64_t)k * c_in + ci) * c_out;
  if (TR) {
    // co = cob * 16 * NB + 16 * n + i16 with i16 = lane & 15: four consecutive output channels
    const int co = cob * (16 * NB) + 16 * n + (lane0 & 15);
    if ((c_out % 4) == 0 && co + 3 < c_out) {
      *reinterpret_cast<f32x4 *>(row + co) = s;
    } else {
#pragma unroll
      for (int t = 0; t < 4; ++t)
        if (co + t < c_out) row[co + t] = s[t];
    }
  } else {
#pragma unroll
    for (int t = 0; t < 4; ++t) {
      const int co = cob * (16 * NB) + NB * ((lane0 + t) & 15) + n;
      if (co < c_out) row[co] = s[t];
    }
  }
}

// ---- the reduce as the tail of another launch ----------------------------------------------------------------------
// Kernel argument of k_conv_tile_f32x3_ws<..., TAIL = true>: the reduce of the split fp32 weight gradient
// (k_wgrad_f32x3: TR images, MB = kWgMB, nb = 1 | 2), done by the workgroups behind the launch's n_tiles tiles.
struct WgTail {
  WgReduceArgs r;
  int nb;        // 16-column blocks per wave of the images (1 | 2)
  int n_tiles;   // workgroups [0, n_tiles) of grid.x are tiles, the rest reduce
};

// image blocks of 256 floats per offset (the images are whole multiples of 256 floats) and groups in all
static inline int64_t wgrad_tail_groups(const WgTail &t) {
  return (int64_t)t.r.n_cib * t.r.n_cob * (kWgMB * t.nb * 4 * 64 / kWgReduceGroup) * t.r.volume;
}

// One workgroup of NT threads serves NT / 256 consecutive groups (group g: offset g / nx, image block g % nx).
// smem: the launch's dynamic LDS (a tail workgroup has no tile), at least (NT / 256) * kWgReduceGroupLds bytes.
// Not inlined: the tile path of the kernel that calls it must not change with it.
template <int NT>
__device__ __noinline__ void wgrad_reduce_tail(WgReduceArgs a, int nb, int tail_block, char *smem) {
  static_assert(NT % kWgReduceGroup == 0, "whole groups");
  constexpr int G = NT / kWgReduceGroup;
  const int tid = threadIdx.x;
  const int grp = tid / kWgReduceGroup;
  const int nx = a.n_cib * a.n_cob * (kWgMB * nb * 4 * 64 / kWgReduceGroup);
  const int64_t g = (int64_t)tail_block * G + grp;
  const bool live = g < (int64_t)nx * a.volume;
  const int k = live ? (int)(g / nx) : 0;
  const int xb = live ? (int)(g % nx) : 0;
  char *mine = smem + grp * kWgReduceGroupLds;
  int64_t *s_r = reinterpret_cast<int64_t *>(mine);
  f32x4 *s_part = reinterpret_cast<f32x4 *>(mine + 64);
  if (nb == 1) wgrad_reduce_group<1, true, kWgMB>(a, k, xb, tid, live, s_r, s_part);
  else wgrad_reduce_group<2, true, kWgMB>(a, k, xb, tid, live, s_r, s_part);
}

// conv.hip: the reduce arguments of the split fp32 weight gradient of a (c_in -> c_out) layer over `workspace`
// (false: that layer's weight gradient is not the split kernel)
bool wgrad_split_tail(const int64_t *k_offsets, const int64_t *k_offsets_dev, int64_t volume, int c_in, int c_out,
                      const void *workspace, float *grad_w, WgTail *tail);

}  // namespace me
