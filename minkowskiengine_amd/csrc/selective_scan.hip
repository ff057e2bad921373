// Selective state-space scan (Mamba S6) over the serialized voxel order, for gfx950 (MI355X): MinkowskiMamba,
// MinkowskiFunctional.selective_scan (ABI 1.27).  Position p of the sequence is row seg_rows[p] (seg_rows[n - 1 - p] with
// `reverse`): every instance along its curve, the instances one after the other (manager._patch_rows with patches of one
// row).  A position whose row belongs to another instance than the position before it (and position 0) RESETS the state:
//   dt   = delta[row, d] + delta_bias[d]                       (softplus of that, torch's threshold form, when asked)
//   h[s] = exp(dt A[d, s]) h[s] + dt u[row, d] B[row, s]       (h = 0 before a reset position)
//   y    = sum_s C[row, s] h[s] + Dskip[d] u[row, d];    out[row, d] = y silu(z[row, d])   (no factor without z)
// Everything is fp32 in registers; bf16 rows are rounded once at the store.
//
// Work split.  A lane owns one channel d and keeps its S states in registers; a workgroup is W waves = 64 W consecutive
// channels (a slab) and walks chunks of kChunk = 64 positions.  The chunks are global (chunk c is positions 64 c ..), so
// the chunk count is ceil(n / 64) without a read-back; the reset flags stand for the instance bounds.  The rows of a
// chunk, their flags and B[row] / C[row] (fp32) are staged once per chunk in LDS by the whole workgroup; the step loop
// reads B / C as LDS broadcasts and u / delta / z as coalesced row reads, kSub = 8 positions ahead in registers.
//   forward   k_sscan_fwd<.., false>  from h = 0: the chunk's end state [chunk, d, s], sum dt [chunk, d], "a reset occurred"
//             k_sscan_carry           entry[c + 1] = reset_c ? end_c : exp(A sum dt_c) entry[c] + end_c, one thread per
//                                     ((d, s), group of consecutive chunks): compose the group, combine the kCarryGroups
//                                     groups in ascending order through LDS, walk the group again from its true entry
//             k_sscan_fwd<.., true>   every chunk again from entry[c]: writes out
//   backward  k_sscan_bwd_state       the chunk walked backwards from e = 0: e = gradient arriving at h_{t-1},
//                                     g = dy C + e,  e <- reset_t ? 0 : exp(dt A) g;  leaves e of the chunk's first position
//             k_sscan_carry (rev)     the same composition over descending chunks: gend[c] = e arriving at the chunk's end
//             k_sscan_bwd_main        see below
//             k_sscan_merge_bc, k_sscan_param_reduce   the fixed-order merges
// entry [chunks, d, s] is all that the forward pass keeps for the backward pass; no [n, d, s] tensor exists anywhere.
//
// Two checkpoint levels.  The backward step needs h_{t-1} next to g_t, and the states of a chunk (64 x S x 4 bytes a lane)
// fit neither registers nor LDS.  k_sscan_bwd_main walks the chunk forwards once from entry[c] and leaves the state before
// every sub-chunk of kSub = 8 positions in LDS (8 x S floats a lane: 32 KiB a wave at S = 16); then, sub-chunk by
// sub-chunk backwards, it recomputes the 8 states of the sub-chunk into registers (8 S of them) and runs the 8 backward
// steps on them.  The recurrence is never inverted (h_{t-1} = (h_t - x B) / a loses everything where a underflows).
//
// dB[t, s] = sum_d g[s] dt u and dC[t, s] = sum_d dy h[s] are sums over the channels, which are lanes: 2 S values a lane and
// step.  They are summed by a transposing butterfly (lane_transpose_sum): stage k exchanges half of the values that a lane
// still holds with lane ^ (1 << k), so the value count halves while the partner count doubles: 2 S - 1 exchanges for the first
// log2(2 S) stages instead of 6 x 2 S for one butterfly a value, and lane L ends with the sum of value slot(L).  The wave
// writes its 2 S sums of the step to LDS; at the end of the chunk the workgroup adds its waves in ascending order and
// writes [slab][position][2 S] to the workspace; k_sscan_merge_bc adds the slabs in ascending order and scatters to the
// rows.  dA, dDskip and ddelta_bias stay in registers over a workgroup's contiguous run of chunks (at most kMaxRuns runs)
// and k_sscan_param_reduce adds the runs in ascending order.  No atomics: every output is bitwise reproducible.
#include "common.hpp"
#include "piece.hpp"

namespace me {
namespace sscan {

constexpr int kChunk = 64;          // positions a chunk (me_sscan_chunk)
constexpr int kSub = 8;             // positions a sub-chunk: the register checkpoint level
constexpr int kNSub = kChunk / kSub;
constexpr int kCarryGroups = 8;     // chunk groups of the carry kernel
constexpr int kMaxRuns = 256;       // runs of chunks of k_sscan_bwd_main: partial records of the parameter gradients

struct Seq {                        // what every pass reads
  const void *u, *delta, *z, *B, *C;
  int64_t u_stride, delta_stride, z_stride, b_stride, c_stride;
  const float *A, *Dskip, *bias;
  const int32_t *seg_rows, *batch_row;
  int64_t n;
  int32_t d, softplus, reverse;
};

struct FwdArgs {
  Seq q;
  float *entry;                     // [chunks, d, s]: written by the carry, read by the OUT pass
  void *out;
  int64_t out_stride;
  float *hend, *sumdt;              // state pass: [chunks, d, s], [chunks, d]
  int32_t *creset;                  // [chunks]
};

struct BwdArgs {
  Seq q;
  const void *dout;
  int64_t dout_stride;
  const float *entry;               // [chunks, d, s] of the forward pass
  float *gend;                      // [chunks, d, s]: written by the reverse carry
  void *du, *ddelta, *dz;           // [n, d] contiguous, each may be NULL
  float *gloc, *sumdt;              // state pass
  int32_t *creset;
  float *bcpart;                    // [slabs][n][2 s], NULL when neither dB nor dC is wanted
  float *ppart;                     // [runs][d][s + 2]
  int32_t nchunks, run_chunks;
};

__device__ __forceinline__ float softplus_f(float x) { return x > 20.f ? x : log1pf(expf(x)); }
__device__ __forceinline__ float sigmoid_f(float x) { return 1.f / (1.f + expf(-x)); }

// rows and reset flags of the chunk at position c0, then B | C of its rows as fp32 [kChunk][2 S] (zeros past nt)
template <typename T, int S, int NT>
__device__ __forceinline__ void stage_chunk(const Seq &q, int64_t c0, int nt, int32_t *rowv, int32_t *flagv, float *bc) {
  for (int t = threadIdx.x; t < kChunk; t += NT) {
    int32_t row = 0, flag = 0;
    if (t < nt) {
      const int64_t p = c0 + t;
      row = q.seg_rows[q.reverse ? q.n - 1 - p : p];
      flag = 1;
      if (p > 0) {
        const int32_t prev = q.seg_rows[q.reverse ? q.n - p : p - 1];
        flag = q.batch_row[row] != q.batch_row[prev] ? 1 : 0;
      }
    }
    rowv[t] = row;
    flagv[t] = flag;
  }
  __syncthreads();
  const T *B = (const T *)q.B, *C = (const T *)q.C;
  for (int i = threadIdx.x; i < kChunk * 2 * S; i += NT) {
    const int t = i / (2 * S), j = i % (2 * S);
    float v = 0.f;
    if (t < nt) {
      const int64_t row = rowv[t];
      v = j < S ? (float)B[row * q.b_stride + j] : (float)C[row * q.c_stride + (j - S)];
    }
    bc[i] = v;
  }
  __syncthreads();
}

// OUT = false: the chunk from h = 0 -> hend, sumdt, creset.  OUT = true: the chunk from entry -> out.
template <typename T, int S, int W, bool OUT>
__global__ __launch_bounds__(64 * W) void k_sscan_fwd(FwdArgs a) {
  constexpr int NT = 64 * W;
  __shared__ int32_t rowv[kChunk], flagv[kChunk];
  __shared__ float bc[kChunk * 2 * S];
  const Seq &q = a.q;
  const int64_t chunk = blockIdx.x, c0 = chunk * kChunk;
  const int nt = (int)(q.n - c0 < kChunk ? q.n - c0 : kChunk);
  const int d = blockIdx.y * NT + threadIdx.x;
  const bool on = d < q.d;
  stage_chunk<T, S, NT>(q, c0, nt, rowv, flagv, bc);
  const T *u = (const T *)q.u, *delta = (const T *)q.delta, *z = (const T *)q.z;
  float A[S], h[S];
#pragma unroll
  for (int s = 0; s < S; ++s) {
    A[s] = on ? q.A[(int64_t)d * S + s] : 0.f;
    h[s] = (OUT && on) ? a.entry[(chunk * q.d + d) * S + s] : 0.f;
  }
  const float bias = (on && q.bias != nullptr) ? q.bias[d] : 0.f;
  const float dsk = (OUT && on && q.Dskip != nullptr) ? q.Dskip[d] : 0.f;
  float sumdt = 0.f;
  int saw = 0;
  for (int t0 = 0; t0 < nt; t0 += kSub) {
    float uv[kSub], dv[kSub], zv[kSub];
#pragma unroll
    for (int k = 0; k < kSub; ++k) {
      uv[k] = dv[k] = zv[k] = 0.f;
      if (on && t0 + k < nt) {
        const int64_t row = rowv[t0 + k];
        uv[k] = (float)u[row * q.u_stride + d];
        dv[k] = (float)delta[row * q.delta_stride + d];
        if (OUT && z != nullptr) zv[k] = (float)z[row * q.z_stride + d];
      }
    }
#pragma unroll
    for (int k = 0; k < kSub; ++k) {
      const int t = t0 + k;
      if (t < nt) {
        if (flagv[t]) {
#pragma unroll
          for (int s = 0; s < S; ++s) h[s] = 0.f;
          sumdt = 0.f;
          saw = 1;
        }
        float dt = dv[k] + bias;
        if (q.softplus) dt = softplus_f(dt);
        const float x = dt * uv[k];
        float y = dsk * uv[k];
        const float *bt = bc + t * 2 * S;
#pragma unroll
        for (int s = 0; s < S; ++s) {
          h[s] = expf(dt * A[s]) * h[s] + x * bt[s];
          if (OUT) y += bt[S + s] * h[s];
        }
        sumdt += dt;
        if (OUT && on) {
          if (z != nullptr) y *= zv[k] * sigmoid_f(zv[k]);
          ((T *)a.out)[(int64_t)rowv[t] * a.out_stride + d] = (T)y;
        }
      }
    }
  }
  if (!OUT && on) {
#pragma unroll
    for (int s = 0; s < S; ++s) a.hend[(chunk * q.d + d) * S + s] = h[s];
    a.sumdt[chunk * q.d + d] = sumdt;
    if (d == 0) a.creset[chunk] = saw;
  }
}

// state[i + 1] = reset_i ? loc_i : exp(A sum dt_i) state[i] + loc_i over the chunks in walking order (i = c, or
// i = chunks - 1 - c with rev), state[0] = 0; entry[c] = the state before chunk c is walked.
__global__ __launch_bounds__(64 * kCarryGroups) void k_sscan_carry(const float *__restrict__ loc,
                                                                  const float *__restrict__ sumdt,
                                                                  const int32_t *__restrict__ creset,
                                                                  const float *__restrict__ A, int nchunks, int ds, int S,
                                                                  int rev, float *__restrict__ entry) {
  __shared__ float sa[kCarryGroups][64], sb[kCarryGroups][64];
  const int x = threadIdx.x & 63, g = threadIdx.x >> 6;
  const int pair = blockIdx.x * 64 + x;
  const bool on = pair < ds;
  const int D = ds / S, d = on ? pair / S : 0;
  const int L = (nchunks + kCarryGroups - 1) / kCarryGroups;
  const int i0 = g * L < nchunks ? g * L : nchunks, i1 = i0 + L < nchunks ? i0 + L : nchunks;
  const float av = on ? A[pair] : 0.f;
  float b = 0.f, sd = 0.f;
  bool cut = false;
  if (on) {
    for (int i = i0; i < i1; ++i) {
      const int64_t c = rev ? nchunks - 1 - i : i;
      const float l = loc[c * ds + pair], sdt = sumdt[c * D + d];
      if (creset[c]) {
        b = l;
        cut = true;
      } else {
        b = expf(av * sdt) * b + l;
        sd += sdt;
      }
    }
  }
  sa[g][x] = cut ? 0.f : expf(av * sd);
  sb[g][x] = b;
  __syncthreads();
  if (!on) return;
  float e = 0.f;
  for (int gg = 0; gg < g; ++gg) e = sa[gg][x] * e + sb[gg][x];
  for (int i = i0; i < i1; ++i) {
    const int64_t c = rev ? nchunks - 1 - i : i;
    entry[c * ds + pair] = e;
    const float l = loc[c * ds + pair], sdt = sumdt[c * D + d];
    e = creset[c] ? l : expf(av * sdt) * e + l;
  }
}

// dy of one position from dout and z
__device__ __forceinline__ float dy_of(float g, float z, bool has_z) { return has_z ? g * z * sigmoid_f(z) : g; }

// the chunk walked backwards from e = 0 -> gloc (e leaving the chunk), sumdt, creset
template <typename T, int S, int W>
__global__ __launch_bounds__(64 * W) void k_sscan_bwd_state(BwdArgs a) {
  constexpr int NT = 64 * W;
  __shared__ int32_t rowv[kChunk], flagv[kChunk];
  __shared__ float bc[kChunk * 2 * S];
  const Seq &q = a.q;
  const int64_t chunk = blockIdx.x, c0 = chunk * kChunk;
  const int nt = (int)(q.n - c0 < kChunk ? q.n - c0 : kChunk);
  const int d = blockIdx.y * NT + threadIdx.x;
  const bool on = d < q.d;
  stage_chunk<T, S, NT>(q, c0, nt, rowv, flagv, bc);
  const T *delta = (const T *)q.delta, *z = (const T *)q.z, *dout = (const T *)a.dout;
  float A[S], e[S];
#pragma unroll
  for (int s = 0; s < S; ++s) {
    A[s] = on ? q.A[(int64_t)d * S + s] : 0.f;
    e[s] = 0.f;
  }
  const float bias = (on && q.bias != nullptr) ? q.bias[d] : 0.f;
  float sumdt = 0.f;
  int saw = 0;
  for (int t0 = (nt - 1) / kSub * kSub; t0 >= 0; t0 -= kSub) {
    float dv[kSub], zv[kSub], gv[kSub];
#pragma unroll
    for (int k = 0; k < kSub; ++k) {
      dv[k] = zv[k] = gv[k] = 0.f;
      if (on && t0 + k < nt) {
        const int64_t row = rowv[t0 + k];
        dv[k] = (float)delta[row * q.delta_stride + d];
        gv[k] = (float)dout[row * a.dout_stride + d];
        if (z != nullptr) zv[k] = (float)z[row * q.z_stride + d];
      }
    }
#pragma unroll
    for (int k = kSub - 1; k >= 0; --k) {
      const int t = t0 + k;
      if (t < nt) {
        float dt = dv[k] + bias;
        if (q.softplus) dt = softplus_f(dt);
        const float dy = dy_of(gv[k], zv[k], z != nullptr);
        const float *ct = bc + t * 2 * S + S;
        const bool flag = flagv[t] != 0;
#pragma unroll
        for (int s = 0; s < S; ++s) e[s] = flag ? 0.f : expf(dt * A[s]) * (dy * ct[s] + e[s]);
        sumdt += dt;
        if (flag) saw = 1;
      }
    }
  }
  if (on) {
#pragma unroll
    for (int s = 0; s < S; ++s) a.gloc[(chunk * q.d + d) * S + s] = e[s];
    a.sumdt[chunk * q.d + d] = sumdt;
    if (d == 0) a.creset[chunk] = saw;
  }
}

// v[j] of every lane -> the sum over the 64 lanes of v[slot], slot = transpose_slot<NV>(lane), in every lane
template <int NV>
__device__ __forceinline__ float lane_transpose_sum(float (&v)[NV]) {
  const int lane = lane_id();
  int k = 0;
#pragma unroll
  for (int half = NV / 2; half >= 1; half >>= 1, ++k) {
    const bool up = (lane >> k) & 1;
#pragma unroll
    for (int i = 0; i < half; ++i) {
      const float keep = up ? v[i + half] : v[i], send = up ? v[i] : v[i + half];
      v[i] = keep + __shfl_xor(send, 1 << k, 64);
    }
  }
  float r = v[0];
  for (; k < 6; ++k) r += __shfl_xor(r, 1 << k, 64);
  return r;
}
template <int NV>
__device__ __forceinline__ int transpose_slot(int lane) {
  int slot = 0, k = 0;
#pragma unroll
  for (int half = NV / 2; half >= 1; half >>= 1, ++k) slot += ((lane >> k) & 1) * half;
  return slot;
}

// a run of chunks: the states recomputed on two checkpoint levels, every gradient but the fixed-order merges
template <typename T, int S, int W>
__global__ __launch_bounds__(64 * W) void k_sscan_bwd_main(BwdArgs a) {
  constexpr int NT = 64 * W;
  __shared__ int32_t rowv[kChunk], flagv[kChunk];
  __shared__ float bc[kChunk * 2 * S];
  __shared__ float ck[kNSub][S][NT];          // the state before every sub-chunk
  __shared__ float red[W][kChunk][2 * S];     // dB | dC of every position, one record a wave
  const Seq &q = a.q;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int d = blockIdx.y * NT + tid;
  const bool on = d < q.d;
  const T *u = (const T *)q.u, *delta = (const T *)q.delta, *z = (const T *)q.z, *dout = (const T *)a.dout;
  const bool has_z = z != nullptr;
  const int slot = transpose_slot<2 * S>(lane);
  float A[S], dA[S];
#pragma unroll
  for (int s = 0; s < S; ++s) {
    A[s] = on ? q.A[(int64_t)d * S + s] : 0.f;
    dA[s] = 0.f;
  }
  const float bias = (on && q.bias != nullptr) ? q.bias[d] : 0.f;
  const float dsk = (on && q.Dskip != nullptr) ? q.Dskip[d] : 0.f;
  float dD = 0.f, dbias = 0.f;
  const int64_t first = (int64_t)blockIdx.x * a.run_chunks;
  const int64_t last = first + a.run_chunks < a.nchunks ? first + a.run_chunks : a.nchunks;
  for (int64_t chunk = first; chunk < last; ++chunk) {
    const int64_t c0 = chunk * kChunk;
    const int nt = (int)(q.n - c0 < kChunk ? q.n - c0 : kChunk);
    const int nsub = (nt + kSub - 1) / kSub;
    __syncthreads();                          // the chunk before has been read out of LDS
    stage_chunk<T, S, NT>(q, c0, nt, rowv, flagv, bc);
    float h[S], e[S];
#pragma unroll
    for (int s = 0; s < S; ++s) {
      h[s] = on ? a.entry[(chunk * q.d + d) * S + s] : 0.f;
      e[s] = on ? a.gend[(chunk * q.d + d) * S + s] : 0.f;
    }
    // level 1: forwards, the state before every sub-chunk to LDS (the last sub-chunk is not walked here)
    for (int sb = 0; sb < nsub; ++sb) {
#pragma unroll
      for (int s = 0; s < S; ++s) ck[sb][s][tid] = h[s];
      if (sb == nsub - 1) break;
      float uv[kSub], dv[kSub];
#pragma unroll
      for (int k = 0; k < kSub; ++k) {
        uv[k] = dv[k] = 0.f;
        if (on) {
          const int64_t row = rowv[sb * kSub + k];
          uv[k] = (float)u[row * q.u_stride + d];
          dv[k] = (float)delta[row * q.delta_stride + d];
        }
      }
#pragma unroll
      for (int k = 0; k < kSub; ++k) {
        const int t = sb * kSub + k;
        float dt = dv[k] + bias;
        if (q.softplus) dt = softplus_f(dt);
        const float x = dt * uv[k];
        const float *bt = bc + t * 2 * S;
        const bool flag = flagv[t] != 0;
#pragma unroll
        for (int s = 0; s < S; ++s) h[s] = expf(dt * A[s]) * (flag ? 0.f : h[s]) + x * bt[s];
      }
    }
    // level 2: backwards over the sub-chunks, the states of one sub-chunk in registers
    for (int sb = nsub - 1; sb >= 0; --sb) {
      float uv[kSub], dv[kSub], zv[kSub], gv[kSub], dtv[kSub], hs[kSub][S];
#pragma unroll
      for (int k = 0; k < kSub; ++k) {
        uv[k] = dv[k] = zv[k] = gv[k] = 0.f;
        if (on && sb * kSub + k < nt) {
          const int64_t row = rowv[sb * kSub + k];
          uv[k] = (float)u[row * q.u_stride + d];
          dv[k] = (float)delta[row * q.delta_stride + d];
          gv[k] = (float)dout[row * a.dout_stride + d];
          if (has_z) zv[k] = (float)z[row * q.z_stride + d];
        }
      }
#pragma unroll
      for (int s = 0; s < S; ++s) h[s] = ck[sb][s][tid];
#pragma unroll
      for (int k = 0; k < kSub; ++k) {
        const int t = sb * kSub + k;
        dv[k] += bias;
        dtv[k] = q.softplus ? softplus_f(dv[k]) : dv[k];
        if (t < nt) {
          const float x = dtv[k] * uv[k];
          const float *bt = bc + t * 2 * S;
          const bool flag = flagv[t] != 0;
#pragma unroll
          for (int s = 0; s < S; ++s) h[s] = expf(dtv[k] * A[s]) * (flag ? 0.f : h[s]) + x * bt[s];
        }
#pragma unroll
        for (int s = 0; s < S; ++s) hs[k][s] = h[s];
      }
#pragma unroll
      for (int k = kSub - 1; k >= 0; --k) {
        const int t = sb * kSub + k;
        if (t < nt) {
          const float *bt = bc + t * 2 * S;
          const bool flag = flagv[t] != 0;
          const float dt = dtv[k], uu = uv[k], x = dt * uu;
          float y = dsk * uu;
#pragma unroll
          for (int s = 0; s < S; ++s) y += bt[S + s] * hs[k][s];
          float dy = gv[k], dzv = 0.f;
          if (has_z) {
            const float sig = sigmoid_f(zv[k]);
            dy = gv[k] * zv[k] * sig;
            dzv = gv[k] * y * sig * (1.f + zv[k] * (1.f - sig));
          }
          dD += dy * uu;
          float dx = 0.f, ddt = 0.f, vbc[2 * S];
#pragma unroll
          for (int s = 0; s < S; ++s) {
            float hp = 0.f;                   // h_{t-1}
            if (!flag) {
              if (k == 0) hp = ck[sb][s][tid];
              else hp = hs[k > 0 ? k - 1 : 0][s];
            }
            const float gs = dy * bt[S + s] + e[s];
            const float av = expf(dt * A[s]);
            vbc[s] = gs * x;
            vbc[S + s] = dy * hs[k][s];
            dx += gs * bt[s];
            const float t1 = gs * hp * av;
            ddt += t1 * A[s];
            dA[s] += t1 * dt;
            e[s] = flag ? 0.f : av * gs;
          }
          ddt += dx * uu;
          const float ddl = (q.softplus && dv[k] <= 20.f) ? ddt * sigmoid_f(dv[k]) : ddt;
          dbias += on ? ddl : 0.f;
          if (on) {
            const int64_t o = (int64_t)rowv[t] * q.d + d;
            if (a.du != nullptr) ((T *)a.du)[o] = (T)(dx * dt + dsk * dy);
            if (a.ddelta != nullptr) ((T *)a.ddelta)[o] = (T)ddl;
            if (a.dz != nullptr) ((T *)a.dz)[o] = (T)dzv;
          }
          if (a.bcpart != nullptr) {
            const float r = lane_transpose_sum<2 * S>(vbc);
            if (lane < 2 * S) red[wave][t][slot] = r;
          }
        }
      }
    }
    if (a.bcpart != nullptr) {
      __syncthreads();
      float *dst = a.bcpart + ((int64_t)blockIdx.y * q.n + c0) * (2 * S);
      for (int i = tid; i < nt * 2 * S; i += NT) {
        float r = (&red[0][0][0])[i];
#pragma unroll
        for (int w = 1; w < W; ++w) r += (&red[w][0][0])[i];
        dst[i] = r;
      }
    }
  }
  if (on) {
    float *p = a.ppart + ((int64_t)blockIdx.x * q.d + d) * (S + 2);
#pragma unroll
    for (int s = 0; s < S; ++s) p[s] = dA[s];
    p[S] = dD;
    p[S + 1] = dbias;
  }
}

// dB[row, s] / dC[row, s] = the slabs' records of the row's position, added in ascending slab order
template <typename T>
__global__ __launch_bounds__(256) void k_sscan_merge_bc(const float *__restrict__ part, int nslab, int64_t n, int S,
                                                        const int32_t *__restrict__ seg_rows, int reverse,
                                                        T *__restrict__ dB, T *__restrict__ dC) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n * 2 * S) return;
  const int64_t p = i / (2 * S);
  const int j = (int)(i % (2 * S));
  float r = part[i];
  for (int sl = 1; sl < nslab; ++sl) r += part[(int64_t)sl * n * 2 * S + i];
  const int64_t row = seg_rows[reverse ? n - 1 - p : p];
  if (j < S) {
    if (dB != nullptr) dB[row * S + j] = (T)r;
  } else if (dC != nullptr) {
    dC[row * S + (j - S)] = (T)r;
  }
}

// dA [d, s], dDskip [d], ddelta_bias [d] = the runs' records, added in ascending run order
__global__ __launch_bounds__(256) void k_sscan_param_reduce(const float *__restrict__ part, int nruns, int d, int S,
                                                            float *__restrict__ dA, float *__restrict__ dD,
                                                            float *__restrict__ dbias) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int64_t rec = (int64_t)d * (S + 2);
  if (i >= rec) return;
  float r = 0.f;
  for (int run = 0; run < nruns; ++run) r += part[run * rec + i];
  const int ch = (int)(i / (S + 2)), j = (int)(i % (S + 2));
  if (j < S) {
    if (dA != nullptr) dA[(int64_t)ch * S + j] = r;
  } else if (j == S) {
    if (dD != nullptr) dD[ch] = r;
  } else if (dbias != nullptr) {
    dbias[ch] = r;
  }
}

// ---- launch policy (host) -------------------------------------------------------------------------------------------
inline int64_t chunks_of(int64_t n) { return ceil_div(n, kChunk); }
inline int fwd_waves(int d) { return d <= 64 ? 1 : d <= 128 ? 2 : 4; }
// the sub-chunk checkpoints are 2 KiB x S a wave: one wave at S = 16, up to two at S = 8 keep a workgroup below 64 KiB
inline int bwd_waves(int d, int s) { return (s == 16 || d <= 64) ? 1 : 2; }
inline int slabs_of(int d, int waves) { return (int)ceil_div(d, 64 * waves); }
inline int run_chunks_of(int64_t nchunks) { return (int)ceil_div(nchunks, kMaxRuns); }

struct Workspace {                  // offsets in floats
  int64_t loc, sumdt, creset, gend, bcpart, ppart, total;
};
inline Workspace workspace_of(int64_t n, int d, int s, bool backward) {
  Workspace w{};
  const int64_t nch = chunks_of(n);
  int64_t o = 0;
  w.loc = o, o += nch * d * s;
  w.sumdt = o, o += nch * d;
  w.creset = o, o += nch;
  if (backward) {
    const int64_t nruns = ceil_div(nch, run_chunks_of(nch));
    w.gend = o, o += nch * d * s;
    w.bcpart = o, o += (int64_t)slabs_of(d, bwd_waves(d, s)) * n * 2 * s;
    w.ppart = o, o += nruns * d * (s + 2);
  }
  w.total = o;
  return w;
}

#define ME_SSCAN_W(T, S, w, KERNEL, ...)                                       \
  switch (w) {                                                                 \
    case 1: hipLaunchKernelGGL((KERNEL<T, S, 1, ##__VA_ARGS__>), dim3(gx, gy), dim3(64), 0, stream, a); break;   \
    case 2: hipLaunchKernelGGL((KERNEL<T, S, 2, ##__VA_ARGS__>), dim3(gx, gy), dim3(128), 0, stream, a); break;  \
    default: hipLaunchKernelGGL((KERNEL<T, S, 4, ##__VA_ARGS__>), dim3(gx, gy), dim3(256), 0, stream, a); break; \
  }

template <typename T, int S>
int forward(FwdArgs a, hipStream_t stream) {
  const Seq &q = a.q;
  const int w = fwd_waves(q.d);
  const unsigned gx = (unsigned)chunks_of(q.n), gy = (unsigned)slabs_of(q.d, w);
  ME_SSCAN_W(T, S, w, k_sscan_fwd, false);
  ME_LAUNCH_CHECK();
  hipLaunchKernelGGL(k_sscan_carry, dim3((unsigned)ceil_div((int64_t)q.d * S, 64)), dim3(64 * kCarryGroups), 0, stream,
                     a.hend, a.sumdt, a.creset, q.A, (int)gx, q.d * S, S, 0, a.entry);
  ME_LAUNCH_CHECK();
  ME_SSCAN_W(T, S, w, k_sscan_fwd, true);
  ME_LAUNCH_CHECK();
  return 0;
}

template <typename T, int S>
int backward(BwdArgs a, void *dB, void *dC, float *dA, float *dD, float *dbias, hipStream_t stream) {
  const Seq &q = a.q;
  const int w = bwd_waves(q.d, S);                     // two waves only at S = 8
  const int nslab = slabs_of(q.d, w);
  unsigned gx = (unsigned)a.nchunks, gy = (unsigned)nslab;
  if (w == 1) hipLaunchKernelGGL((k_sscan_bwd_state<T, S, 1>), dim3(gx, gy), dim3(64), 0, stream, a);
  else if constexpr (S == 8) hipLaunchKernelGGL((k_sscan_bwd_state<T, S, 2>), dim3(gx, gy), dim3(128), 0, stream, a);
  ME_LAUNCH_CHECK();
  hipLaunchKernelGGL(k_sscan_carry, dim3((unsigned)ceil_div((int64_t)q.d * S, 64)), dim3(64 * kCarryGroups), 0, stream,
                     a.gloc, a.sumdt, a.creset, q.A, a.nchunks, q.d * S, S, 1, a.gend);
  ME_LAUNCH_CHECK();
  const int nruns = (int)ceil_div(a.nchunks, a.run_chunks);
  gx = (unsigned)nruns;
  if (w == 1) hipLaunchKernelGGL((k_sscan_bwd_main<T, S, 1>), dim3(gx, gy), dim3(64), 0, stream, a);
  else if constexpr (S == 8) hipLaunchKernelGGL((k_sscan_bwd_main<T, S, 2>), dim3(gx, gy), dim3(128), 0, stream, a);
  ME_LAUNCH_CHECK();
  if (a.bcpart != nullptr) {
    hipLaunchKernelGGL(k_sscan_merge_bc<T>, dim3((unsigned)ceil_div(q.n * 2 * S, 256)), dim3(256), 0, stream, a.bcpart,
                       nslab, q.n, S, q.seg_rows, q.reverse, (T *)dB, (T *)dC);
    ME_LAUNCH_CHECK();
  }
  if (dA != nullptr || dD != nullptr || dbias != nullptr) {
    hipLaunchKernelGGL(k_sscan_param_reduce, dim3((unsigned)ceil_div((int64_t)q.d * (S + 2), 256)), dim3(256), 0, stream,
                       a.ppart, nruns, q.d, S, dA, dD, dbias);
    ME_LAUNCH_CHECK();
  }
  return 0;
}

}  // namespace sscan
}  // namespace me

using namespace me;

// the checks both directions share; rows of n > 0 follow in the callers
#define ME_SSCAN_CHECK_SHAPE(n, d, s)                                                                 \
  ME_CHECK(n >= 0 && n < ((int64_t)1 << 31), "n must be in [0, 2^31)");                               \
  ME_CHECK(me_sscan_supported(d, s, 0) != 0, "the kernels serve d >= 1 channels and s = 8 or 16 states")

extern "C" {

int32_t me_sscan_supported(int32_t d, int32_t s, int32_t is_bf16) {
  (void)is_bf16;
  return (d >= 1 && (s == 8 || s == 16)) ? 1 : 0;
}

int32_t me_sscan_chunk(void) { return sscan::kChunk; }

int64_t me_sscan_workspace_bytes(int64_t n, int32_t d, int32_t s, int32_t backward) {
  if (n <= 0 || d < 1 || s < 1) return 0;
  return sscan::workspace_of(n, d, s, backward != 0).total * (int64_t)sizeof(float);
}

int me_sscan_forward(const void *u_dev, const void *delta_dev, const void *z_dev, const void *b_dev, const void *c_dev,
                     int32_t is_bf16, int64_t u_stride, int64_t delta_stride, int64_t z_stride, int64_t b_stride,
                     int64_t c_stride, const float *a_dev, const float *dskip_dev, const float *delta_bias_dev,
                     int32_t delta_softplus, const int32_t *seg_rows_dev, const int32_t *batch_row_dev, int32_t reverse,
                     int64_t n, int32_t d, int32_t s, void *out_dev, int64_t out_stride, float *entry_dev,
                     void *workspace_dev, int64_t workspace_bytes, void *stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  ME_SSCAN_CHECK_SHAPE(n, d, s);
  ME_CHECK(u_stride >= d && delta_stride >= d && (z_dev == nullptr || z_stride >= d) && out_stride >= d,
           "a row stride must be at least d");
  ME_CHECK(b_stride >= s && c_stride >= s, "the row stride of B and C must be at least s");
  if (n == 0) return 0;
  ME_CHECK(u_dev != nullptr && delta_dev != nullptr && b_dev != nullptr && c_dev != nullptr && a_dev != nullptr &&
               out_dev != nullptr && entry_dev != nullptr,
           "u, delta, B, C, A, out and entry must be given");
  ME_CHECK(seg_rows_dev != nullptr && batch_row_dev != nullptr, "the sequence rows and the instance of every row must be given");
  ME_CHECK(workspace_dev != nullptr && workspace_bytes >= me_sscan_workspace_bytes(n, d, s, 0),
           "the workspace is smaller than me_sscan_workspace_bytes");
  const int elem = is_bf16 ? 2 : 4;
  ME_CHECK(aligned({u_dev, delta_dev, z_dev, b_dev, c_dev, out_dev}, elem) &&
               aligned({a_dev, dskip_dev, delta_bias_dev, seg_rows_dev, batch_row_dev, entry_dev, workspace_dev}, 4),
           "the operands must be aligned to their element");
  const sscan::Workspace w = sscan::workspace_of(n, d, s, false);
  float *ws = (float *)workspace_dev;
  const sscan::FwdArgs a{{u_dev, delta_dev, z_dev, b_dev, c_dev, u_stride, delta_stride, z_stride, b_stride, c_stride, a_dev,
                          dskip_dev, delta_bias_dev, seg_rows_dev, batch_row_dev, n, d, delta_softplus ? 1 : 0,
                          reverse ? 1 : 0},
                         entry_dev, out_dev, out_stride, ws + w.loc, ws + w.sumdt, (int32_t *)(ws + w.creset)};
  if (is_bf16) return s == 8 ? sscan::forward<__bf16, 8>(a, stream) : sscan::forward<__bf16, 16>(a, stream);
  return s == 8 ? sscan::forward<float, 8>(a, stream) : sscan::forward<float, 16>(a, stream);
}

int me_sscan_backward(const void *u_dev, const void *delta_dev, const void *z_dev, const void *b_dev, const void *c_dev,
                      const void *dout_dev, int32_t is_bf16, int64_t u_stride, int64_t delta_stride, int64_t z_stride,
                      int64_t b_stride, int64_t c_stride, int64_t dout_stride, const float *a_dev, const float *dskip_dev,
                      const float *delta_bias_dev, int32_t delta_softplus, const int32_t *seg_rows_dev,
                      const int32_t *batch_row_dev, int32_t reverse, int64_t n, int32_t d, int32_t s,
                      const float *entry_dev, void *du_dev, void *ddelta_dev, void *dz_dev, void *db_dev, void *dc_dev,
                      float *da_dev, float *ddskip_dev, float *ddelta_bias_dev, void *workspace_dev,
                      int64_t workspace_bytes, void *stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  ME_SSCAN_CHECK_SHAPE(n, d, s);
  ME_CHECK(u_stride >= d && delta_stride >= d && (z_dev == nullptr || z_stride >= d) && dout_stride >= d,
           "a row stride must be at least d");
  ME_CHECK(b_stride >= s && c_stride >= s, "the row stride of B and C must be at least s");
  ME_CHECK(dz_dev == nullptr || z_dev != nullptr, "dz needs z");
  ME_CHECK(ddskip_dev == nullptr || dskip_dev != nullptr, "the gradient of Dskip needs Dskip");
  ME_CHECK(ddelta_bias_dev == nullptr || delta_bias_dev != nullptr, "the gradient of delta_bias needs delta_bias");
  if (n == 0) {                                       // no rows: the parameter gradients are sums of no records
    if (da_dev != nullptr || ddskip_dev != nullptr || ddelta_bias_dev != nullptr) {
      hipLaunchKernelGGL(sscan::k_sscan_param_reduce, dim3((unsigned)ceil_div((int64_t)d * (s + 2), 256)), dim3(256), 0,
                         stream, (const float *)nullptr, 0, d, s, da_dev, ddskip_dev, ddelta_bias_dev);
      ME_LAUNCH_CHECK();
    }
    return 0;
  }
  ME_CHECK(u_dev != nullptr && delta_dev != nullptr && b_dev != nullptr && c_dev != nullptr && a_dev != nullptr &&
               dout_dev != nullptr && entry_dev != nullptr,
           "u, delta, B, C, A, dout and entry must be given");
  ME_CHECK(seg_rows_dev != nullptr && batch_row_dev != nullptr, "the sequence rows and the instance of every row must be given");
  ME_CHECK(workspace_dev != nullptr && workspace_bytes >= me_sscan_workspace_bytes(n, d, s, 1),
           "the workspace is smaller than me_sscan_workspace_bytes");
  const int elem = is_bf16 ? 2 : 4;
  ME_CHECK(aligned({u_dev, delta_dev, z_dev, b_dev, c_dev, dout_dev, du_dev, ddelta_dev, dz_dev, db_dev, dc_dev}, elem) &&
               aligned({a_dev, dskip_dev, delta_bias_dev, seg_rows_dev, batch_row_dev, entry_dev, da_dev, ddskip_dev,
                        ddelta_bias_dev, workspace_dev}, 4),
           "the operands must be aligned to their element");
  const sscan::Workspace w = sscan::workspace_of(n, d, s, true);
  float *ws = (float *)workspace_dev;
  const int64_t nch = sscan::chunks_of(n);
  const sscan::BwdArgs a{{u_dev, delta_dev, z_dev, b_dev, c_dev, u_stride, delta_stride, z_stride, b_stride, c_stride, a_dev,
                          dskip_dev, delta_bias_dev, seg_rows_dev, batch_row_dev, n, d, delta_softplus ? 1 : 0,
                          reverse ? 1 : 0},
                         dout_dev, dout_stride, entry_dev, ws + w.gend, du_dev, ddelta_dev, dz_dev, ws + w.loc,
                         ws + w.sumdt, (int32_t *)(ws + w.creset),
                         (db_dev != nullptr || dc_dev != nullptr) ? ws + w.bcpart : nullptr, ws + w.ppart, (int32_t)nch,
                         sscan::run_chunks_of(nch)};
  if (is_bf16)
    return s == 8 ? sscan::backward<__bf16, 8>(a, db_dev, dc_dev, da_dev, ddskip_dev, ddelta_bias_dev, stream)
                  : sscan::backward<__bf16, 16>(a, db_dev, dc_dev, da_dev, ddskip_dev, ddelta_bias_dev, stream);
  return s == 8 ? sscan::backward<float, 8>(a, db_dev, dc_dev, da_dev, ddskip_dev, ddelta_bias_dev, stream)
                : sscan::backward<float, 16>(a, db_dev, dc_dev, da_dev, ddskip_dev, ddelta_bias_dev, stream);
}

}  // extern "C"
