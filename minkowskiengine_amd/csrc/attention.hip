// Per-instance multi-head attention over the rows of a coordinate map for gfx950 (MI355X).  q [n_q, H * D] sits on map A,
// k / v [n_kv, H * D] on map B; a query row attends to the key rows with its own batch index and to no others:
//   s_ij = scale * <q_i, k_j>,  out_i = sum_j softmax_j(s_ij) v_j,  lse_i = log sum_j exp(s_ij)   per head.
// The rows of an instance are found through a per-instance row list (seg_ptr int32 [n_batch + 1], seg_rows int32 [n], rows
// ascending inside an instance: me_csr_from_coo of the origin rows), so rows may sit in any order, nothing is padded and the
// host reads nothing back.  Keys are taken in ascending row index: the fixed summation order.
//
//   k_attn_fwd     query-stationary.  A workgroup of two waves owns (instance, head, 64 queries), a wave 32 of them.  It
//                  walks the instance's keys in blocks of 64 with an online softmax in fp32 and writes out / lse once.
//   k_attn_delta   delta[i, h] = <dout_i, out_i> into the workspace (a pre-pass of the backward, read by both kernels below)
//   k_attn_bwd_kv  key-stationary.  A workgroup owns (instance, head, 64 keys) and walks the queries in blocks of 32; P is
//                  recomputed from lse; dV = P^T dO and dK = scale dS^T Q stay in registers and are written once.
//   k_attn_bwd_q   query-stationary.  The same recomputation; dQ = scale dS K in registers, written once.  No atomics: the
//                  second recomputation buys bitwise reproducible gradients.
//
// One 32x32 MFMA shape serves both dtypes: v_mfma_f32_32x32x16_bf16 on bf16 rows, the exact v_mfma_f32_32x32x2_f32 on fp32
// rows; their C/D lane map is the same (column = lane & 31, row = (reg & 3) + 8 (reg >> 2) + 4 (lane >> 5)).  The stationary
// side sits on the LANE of every first product (S^T = K Q^T forward: the query is the column), so
//   * the statistics of a query (running maximum, sum, lse, delta) are per-lane scalars: one cross-lane step (lane ^ 32);
//   * the accumulator of the first product is the B operand of the second with no lane movement and no LDS
//     (O^T += V^T P^T sums over P^T's ROW index): registers 8s .. 8s+7 are k-step s, element j of lane half h being row
//     16 s + 8 (j >> 2) + 4 h + (j & 3).  The A operand of that product is read from a TRANSPOSED LDS image in the same
//     permuted order (two 4-element reads); P and dS are rounded to bf16 there on bf16 rows and stay fp32 on fp32 rows.
// The walked side is staged into LDS in 16-byte pieces through the row list: a natural image [row][D] for the first
// products and a transposed image [D][row] for the second ones.  Partial blocks clamp the row index to the instance's last
// row (a block never reads another instance's rows) and mask the value: a masked key gets the score -inf before the running
// maximum and probability 0, and the operands of the second products are staged as zeros, so no 0 * Inf appears.
// A fragment is 16 k-values: lane half h takes k = 16 c + 8 h + (0 .. 7); on fp32 rows those are eight 32x32x2 steps.
//
// Surplus workgroups: the grid holds ceil(n / block) + n_batch blocks per head, an upper bound of the blocks of all
// instances; a workgroup finds its (instance, block) by walking seg_ptr and exits when there is none.  One launch per kernel.
// The walk is O(instances) dependent loads: fine for a handful of scenes, not for the thousands of patches of serialized
// patch attention (serial_attention.hip), whose lists come with a block table of one (segment, first row) pair per
// workgroup; the _tab entry points take it and the kernels branch on the pointer at entry (k_attn_delta walks nothing).
// The float64 twins at the end are the gradcheck yardstick (plain double, one thread per (row, head)).
#include "attn_block.hpp"
#include "common.hpp"

#include <algorithm>
#include <cmath>

namespace me {

typedef float at_f32x16 __attribute__((ext_vector_type(16)));
typedef float at_f32x4 __attribute__((ext_vector_type(4)));
typedef __bf16 at_bf16x8 __attribute__((ext_vector_type(8)));
typedef __bf16 at_bf16x4 __attribute__((ext_vector_type(4)));

constexpr int kAttnThreads = 128;   // two waves, 32 stationary rows each
constexpr int kAttnFwdWalk = 64;    // key rows staged per step, forward
constexpr int kAttnBwdWalk = 32;    // rows staged per step, backward kernels (two / four images instead of two)

template <typename T> struct AttnT;
template <> struct AttnT<__bf16> {
  typedef at_bf16x8 vec;            // a 16-byte piece
  static constexpr int EPP = 8;     // elements of a 16-byte piece
  static constexpr int PADN = 8;    // natural image: row + 16 B
  static constexpr int PADT = 4;    // transposed image: row + 8 B
};
template <> struct AttnT<float> {
  typedef at_f32x4 vec;
  static constexpr int EPP = 4;
  static constexpr int PADN = 4;
  static constexpr int PADT = 4;
};

// 8 k-values of one operand row
template <typename T> struct AttnFrag;
template <> struct AttnFrag<__bf16> { at_bf16x8 v; };
template <> struct AttnFrag<float> { float v[8]; };

__device__ __forceinline__ void attn_mma(at_f32x16 &acc, const AttnFrag<__bf16> &a, const AttnFrag<__bf16> &b) {
  acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a.v, b.v, acc, 0, 0, 0);
}
__device__ __forceinline__ void attn_mma(at_f32x16 &acc, const AttnFrag<float> &a, const AttnFrag<float> &b) {
#pragma unroll
  for (int j = 0; j < 8; ++j) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a.v[j], b.v[j], acc, 0, 0, 0);
}

// 8 consecutive elements at p (16-byte aligned)
__device__ __forceinline__ AttnFrag<__bf16> attn_load8(const __bf16 *p) {
  AttnFrag<__bf16> f;
  f.v = *reinterpret_cast<const at_bf16x8 *>(p);
  return f;
}
__device__ __forceinline__ AttnFrag<float> attn_load8(const float *p) {
  AttnFrag<float> f;
  const at_f32x4 a = *reinterpret_cast<const at_f32x4 *>(p), b = *reinterpret_cast<const at_f32x4 *>(p + 4);
#pragma unroll
  for (int j = 0; j < 4; ++j) { f.v[j] = a[j]; f.v[4 + j] = b[j]; }
  return f;
}
// elements 0..3 at p, 4..7 at p + 8: the k order of an accumulator used as an operand
__device__ __forceinline__ AttnFrag<__bf16> attn_load44(const __bf16 *p) {
  AttnFrag<__bf16> f;
  const at_bf16x4 a = *reinterpret_cast<const at_bf16x4 *>(p), b = *reinterpret_cast<const at_bf16x4 *>(p + 8);
#pragma unroll
  for (int j = 0; j < 4; ++j) { f.v[j] = a[j]; f.v[4 + j] = b[j]; }
  return f;
}
__device__ __forceinline__ AttnFrag<float> attn_load44(const float *p) {
  AttnFrag<float> f;
  const at_f32x4 a = *reinterpret_cast<const at_f32x4 *>(p), b = *reinterpret_cast<const at_f32x4 *>(p + 8);
#pragma unroll
  for (int j = 0; j < 4; ++j) { f.v[j] = a[j]; f.v[4 + j] = b[j]; }
  return f;
}
// registers 8 s .. 8 s + 7 of a 32x32 tile as the fragment of k-step s
template <typename T>
__device__ __forceinline__ AttnFrag<T> attn_acc_frag(const float (&x)[16], int s) {
  AttnFrag<T> f;
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    if constexpr (sizeof(T) == 2) f.v[j] = (__bf16)x[8 * s + j];
    else f.v[j] = x[8 * s + j];
  }
  return f;
}
// row of register reg of a 32x32 C/D tile in lane half h
__device__ __forceinline__ int attn_row(int reg, int h) { return (reg & 3) + 8 * (reg >> 2) + 4 * h; }

template <typename T> __device__ __forceinline__ float attn_exp(float x) {
  if constexpr (sizeof(T) == 2) return __expf(x);   // P is rounded to bf16 afterwards
  else return expf(x);
}

// (instance, block) of workgroup `blk`: the blocks of the instances in ascending instance order.  With a block table
// (attn_block.hpp) the item is one 8-byte load; without one the workgroup walks seg_ptr.  `tab` is a kernel argument: the
// branch is wave-uniform.
__device__ __forceinline__ bool attn_find_item(const int32_t *__restrict__ tab, const int32_t *__restrict__ seg_ptr,
                                               int n_batch, int blk, int height, int &b, int &t0, int &start, int &len) {
  if (tab != nullptr) {
    b = tab[2 * blk];
    if (b < 0) return false;
    t0 = tab[2 * blk + 1];
    start = seg_ptr[b];
    len = seg_ptr[b + 1] - start;
    return true;
  }
  int acc = 0;
  for (b = 0; b < n_batch; ++b) {
    start = seg_ptr[b];
    len = seg_ptr[b + 1] - start;
    const int nb = (len + height - 1) / height;
    if (blk < acc + nb) {
      t0 = (blk - acc) * height;
      return true;
    }
    acc += nb;
  }
  return false;
}

// Stage W rows x D columns of head `head` into LDS: rows t0 .. t0 + W - 1 of an instance of `len` rows whose row list
// starts at seg_rows[start].  The index of a row past the end is clamped to the last row; its values are written as zeros
// into the transposed image, and into the natural one too when zero_nat.  nat / tr may be null.
template <typename T, int D, int W>
__device__ __forceinline__ void attn_stage(const T *__restrict__ x, int64_t stride, int head,
                                           const int32_t *__restrict__ seg_rows, int start, int len, int t0, T *nat,
                                           bool zero_nat, T *tr) {
  constexpr int EPP = AttnT<T>::EPP, PPR = D / EPP, LDN = D + AttnT<T>::PADN, LDT = W + AttnT<T>::PADT;
  using vec = typename AttnT<T>::vec;
  for (int p = threadIdx.x; p < W * PPR; p += kAttnThreads) {
    const int w = p / PPR, pc = p - w * PPR;
    const bool valid = t0 + w < len;
    const int64_t row = seg_rows[start + min(t0 + w, len - 1)];
    const vec val = *reinterpret_cast<const vec *>(x + row * stride + (int64_t)head * D + pc * EPP);
    vec vz;
#pragma unroll
    for (int j = 0; j < EPP; ++j) vz[j] = valid ? val[j] : (T)0.f;
    if (nat) *reinterpret_cast<vec *>(nat + w * LDN + pc * EPP) = zero_nat ? vz : val;
    if (tr) {
#pragma unroll
      for (int j = 0; j < EPP; ++j) tr[(pc * EPP + j) * LDT + w] = vz[j];
    }
  }
}

// 4 consecutive channels of one row
__device__ __forceinline__ void attn_store4(__bf16 *p, float a, float b, float c, float d) {
  at_bf16x4 v;
  v[0] = (__bf16)a; v[1] = (__bf16)b; v[2] = (__bf16)c; v[3] = (__bf16)d;
  *reinterpret_cast<at_bf16x4 *>(p) = v;
}
__device__ __forceinline__ void attn_store4(float *p, float a, float b, float c, float d) {
  at_f32x4 v;
  v[0] = a; v[1] = b; v[2] = c; v[3] = d;
  *reinterpret_cast<at_f32x4 *>(p) = v;
}

// a transposed accumulator tile set acc[dt][reg] = Y^T[channel dt * 32 + row(reg, h)][stationary row on the lane] times
// `mul`, to row `row` of y
template <typename T, int D>
__device__ __forceinline__ void attn_store_rows(T *__restrict__ y, int64_t stride, int64_t row, int head,
                                                const at_f32x16 (&acc)[D / 32], float mul, int h) {
  T *base = y + row * stride + (int64_t)head * D;
#pragma unroll
  for (int dt = 0; dt < D / 32; ++dt)
#pragma unroll
    for (int g = 0; g < 4; ++g)
      attn_store4(base + dt * 32 + 8 * g + 4 * h, acc[dt][4 * g] * mul, acc[dt][4 * g + 1] * mul, acc[dt][4 * g + 2] * mul,
                  acc[dt][4 * g + 3] * mul);
}

// ---- forward ---------------------------------------------------------------------------------------------------------
template <typename T, int D>
__global__ __launch_bounds__(kAttnThreads) void k_attn_fwd(
    const T *__restrict__ q, const T *__restrict__ k, const T *__restrict__ v, int64_t q_stride, int64_t k_stride,
    int64_t v_stride, const int32_t *__restrict__ seg_ptr_q, const int32_t *__restrict__ seg_rows_q,
    const int32_t *__restrict__ seg_ptr_kv, const int32_t *__restrict__ seg_rows_kv,
    const int32_t *__restrict__ blk_tab, int n_batch, int heads, float scale, T *__restrict__ out, int64_t out_stride,
    float *__restrict__ lse) {
  constexpr int NC = D / 16, ND = D / 32, W = kAttnFwdWalk;
  constexpr int LDN = D + AttnT<T>::PADN, LDT = W + AttnT<T>::PADT;
  extern __shared__ __attribute__((aligned(16))) unsigned char s_attn[];
  T *s_k = reinterpret_cast<T *>(s_attn);   // [W][LDN]
  T *s_vt = s_k + W * LDN;                  // [D][LDT]
  int b, t0, startq, lenq;
  if (!attn_find_item(blk_tab, seg_ptr_q, n_batch, blockIdx.x, kAttnBlock, b, t0, startq, lenq)) return;
  const int head = blockIdx.y;
  const int startk = seg_ptr_kv[b], lenk = seg_ptr_kv[b + 1] - startk;
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, r = lane & 31, h = lane >> 5;
  const int tq = t0 + wave * 32 + r;
  const bool validq = tq < lenq, wave_on = t0 + wave * 32 < lenq;
  const int64_t qi = seg_rows_q[startq + min(tq, lenq - 1)];
  AttnFrag<T> qf[NC];
  {
    const T *qp = q + qi * q_stride + (int64_t)head * D + 8 * h;
#pragma unroll
    for (int c = 0; c < NC; ++c) qf[c] = attn_load8(qp + 16 * c);
  }
  at_f32x16 o[ND];
#pragma unroll
  for (int dt = 0; dt < ND; ++dt)
#pragma unroll
    for (int i = 0; i < 16; ++i) o[dt][i] = 0.f;
  float m = -INFINITY, l = 0.f;
  for (int kb0 = 0; kb0 < lenk; kb0 += W) {
    __syncthreads();
    attn_stage<T, D, W>(k, k_stride, head, seg_rows_kv, startk, lenk, kb0, s_k, false, (T *)nullptr);
    attn_stage<T, D, W>(v, v_stride, head, seg_rows_kv, startk, lenk, kb0, (T *)nullptr, false, s_vt);
    __syncthreads();
    if (!wave_on) continue;
    for (int kbase = 0; kbase < W && kb0 + kbase < lenk; kbase += 32) {
      at_f32x16 s;
#pragma unroll
      for (int i = 0; i < 16; ++i) s[i] = 0.f;
      const T *kp = s_k + (kbase + r) * LDN + 8 * h;
#pragma unroll
      for (int c = 0; c < NC; ++c) attn_mma(s, attn_load8(kp + 16 * c), qf[c]);   // S^T[key][query]
      float x[16], mx = -INFINITY;
#pragma unroll
      for (int i = 0; i < 16; ++i) {
        x[i] = (kb0 + kbase + attn_row(i, h) < lenk) ? s[i] * scale : -INFINITY;
        mx = fmaxf(mx, x[i]);
      }
      mx = fmaxf(mx, __shfl_xor(mx, 32, 64));
      const float m_new = fmaxf(m, mx);
      const float alpha = attn_exp<T>(m - m_new);
      float ps = 0.f;
#pragma unroll
      for (int i = 0; i < 16; ++i) {
        x[i] = attn_exp<T>(x[i] - m_new);
        ps += x[i];
      }
      ps += __shfl_xor(ps, 32, 64);
      l = l * alpha + ps;
      m = m_new;
#pragma unroll
      for (int dt = 0; dt < ND; ++dt)
#pragma unroll
        for (int i = 0; i < 16; ++i) o[dt][i] *= alpha;
#pragma unroll
      for (int s2 = 0; s2 < 2; ++s2) {
        const AttnFrag<T> pf = attn_acc_frag<T>(x, s2);
#pragma unroll
        for (int dt = 0; dt < ND; ++dt)   // O^T[channel][query] += V^T[channel][key] P^T[key][query]
          attn_mma(o[dt], attn_load44(s_vt + (dt * 32 + r) * LDT + kbase + 16 * s2 + 4 * h), pf);
      }
    }
  }
  if (!validq) return;
  attn_store_rows<T, D>(out, out_stride, qi, head, o, l > 0.f ? 1.f / l : 0.f, h);
  if (h == 0) lse[qi * heads + head] = l > 0.f ? m + logf(l) : -INFINITY;
}

// ---- delta[i, h] = <dout_i, out_i> -------------------------------------------------------------------------------------
// The diagonal of the 32x32 product O dO^T of 32 rows, on the MFMA chain the backward kernels use for dP = dO V^T: where a
// query attends to one key (out_i = v_j), dP - delta is then exactly 0.
template <typename T, int D>
__global__ __launch_bounds__(64) void k_attn_delta(const T *__restrict__ out, const T *__restrict__ dout,
                                                   int64_t out_stride, int64_t dout_stride, int64_t n, int heads,
                                                   float *__restrict__ delta) {
  constexpr int NC = D / 16;
  const int lane = threadIdx.x & 63, r = lane & 31, h = lane >> 5, head = blockIdx.y;
  const int64_t row = (int64_t)blockIdx.x * 32 + r, rc = row < n ? row : n - 1;
  const T *op = out + rc * out_stride + (int64_t)head * D + 8 * h;
  const T *gp = dout + rc * dout_stride + (int64_t)head * D + 8 * h;
  at_f32x16 acc;
#pragma unroll
  for (int i = 0; i < 16; ++i) acc[i] = 0.f;
#pragma unroll
  for (int c = 0; c < NC; ++c) attn_mma(acc, attn_load8(op + 16 * c), attn_load8(gp + 16 * c));
  // element [row r][column r] sits in lane half (r >> 2) & 1, register (r & 3) + 4 (r >> 3)
  const int reg = (r & 3) + 4 * (r >> 3);
  float d = 0.f;
#pragma unroll
  for (int i = 0; i < 16; ++i) d = (i == reg) ? acc[i] : d;
  const float other = __shfl_xor(d, 32, 64);
  if (((r >> 2) & 1) != h) d = other;
  if (h == 0 && row < n) delta[row * heads + head] = d;
}

// ---- backward: dQ, query-stationary ----------------------------------------------------------------------------------
template <typename T, int D>
__global__ __launch_bounds__(kAttnThreads) void k_attn_bwd_q(
    const T *__restrict__ q, const T *__restrict__ k, const T *__restrict__ v, const T *__restrict__ dout,
    int64_t q_stride, int64_t k_stride, int64_t v_stride, int64_t dout_stride, const int32_t *__restrict__ seg_ptr_q,
    const int32_t *__restrict__ seg_rows_q, const int32_t *__restrict__ seg_ptr_kv,
    const int32_t *__restrict__ seg_rows_kv, const int32_t *__restrict__ blk_tab, int n_batch, int heads, float scale,
    const float *__restrict__ lse,
    const float *__restrict__ delta, T *__restrict__ dq, int64_t dq_stride) {
  constexpr int NC = D / 16, ND = D / 32, W = kAttnBwdWalk;
  constexpr int LDN = D + AttnT<T>::PADN, LDT = W + AttnT<T>::PADT;
  extern __shared__ __attribute__((aligned(16))) unsigned char s_attn[];
  T *s_k = reinterpret_cast<T *>(s_attn);   // [W][LDN]
  T *s_v = s_k + W * LDN;                   // [W][LDN]
  T *s_kt = s_v + W * LDN;                  // [D][LDT]
  int b, t0, startq, lenq;
  if (!attn_find_item(blk_tab, seg_ptr_q, n_batch, blockIdx.x, kAttnBlock, b, t0, startq, lenq)) return;
  const int head = blockIdx.y;
  const int startk = seg_ptr_kv[b], lenk = seg_ptr_kv[b + 1] - startk;
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, r = lane & 31, h = lane >> 5;
  const int tq = t0 + wave * 32 + r;
  const bool validq = tq < lenq, wave_on = t0 + wave * 32 < lenq;
  const int64_t qi = seg_rows_q[startq + min(tq, lenq - 1)];
  AttnFrag<T> qf[NC], gf[NC];
  {
    const T *qp = q + qi * q_stride + (int64_t)head * D + 8 * h;
    const T *gp = dout + qi * dout_stride + (int64_t)head * D + 8 * h;
#pragma unroll
    for (int c = 0; c < NC; ++c) {
      qf[c] = attn_load8(qp + 16 * c);
      gf[c] = attn_load8(gp + 16 * c);
    }
  }
  const float lse_q = lse[qi * heads + head], delta_q = delta[qi * heads + head];
  at_f32x16 acc[ND];
#pragma unroll
  for (int dt = 0; dt < ND; ++dt)
#pragma unroll
    for (int i = 0; i < 16; ++i) acc[dt][i] = 0.f;
  for (int kb0 = 0; kb0 < lenk; kb0 += W) {
    __syncthreads();
    attn_stage<T, D, W>(k, k_stride, head, seg_rows_kv, startk, lenk, kb0, s_k, false, s_kt);
    attn_stage<T, D, W>(v, v_stride, head, seg_rows_kv, startk, lenk, kb0, s_v, true, (T *)nullptr);
    __syncthreads();
    if (!wave_on) continue;
    at_f32x16 s, dp;
#pragma unroll
    for (int i = 0; i < 16; ++i) { s[i] = 0.f; dp[i] = 0.f; }
    const T *kp = s_k + r * LDN + 8 * h, *vp = s_v + r * LDN + 8 * h;
#pragma unroll
    for (int c = 0; c < NC; ++c) attn_mma(s, attn_load8(kp + 16 * c), qf[c]);    // S^T[key][query]
#pragma unroll
    for (int c = 0; c < NC; ++c) attn_mma(dp, attn_load8(vp + 16 * c), gf[c]);   // dP^T[key][query]
    float ds[16];
#pragma unroll
    for (int i = 0; i < 16; ++i) {
      const float p = (kb0 + attn_row(i, h) < lenk) ? attn_exp<T>(s[i] * scale - lse_q) : 0.f;
      ds[i] = p * (dp[i] - delta_q);
    }
#pragma unroll
    for (int s2 = 0; s2 < 2; ++s2) {
      const AttnFrag<T> df = attn_acc_frag<T>(ds, s2);
#pragma unroll
      for (int dt = 0; dt < ND; ++dt)   // dQ^T[channel][query] += K^T[channel][key] dS^T[key][query]
        attn_mma(acc[dt], attn_load44(s_kt + (dt * 32 + r) * LDT + 16 * s2 + 4 * h), df);
    }
  }
  if (validq) attn_store_rows<T, D>(dq, dq_stride, qi, head, acc, scale, h);
}

// ---- backward: dK / dV, key-stationary -------------------------------------------------------------------------------
template <typename T, int D>
__global__ __launch_bounds__(kAttnThreads) void k_attn_bwd_kv(
    const T *__restrict__ q, const T *__restrict__ k, const T *__restrict__ v, const T *__restrict__ dout,
    int64_t q_stride, int64_t k_stride, int64_t v_stride, int64_t dout_stride, const int32_t *__restrict__ seg_ptr_q,
    const int32_t *__restrict__ seg_rows_q, const int32_t *__restrict__ seg_ptr_kv,
    const int32_t *__restrict__ seg_rows_kv, const int32_t *__restrict__ blk_tab, int n_batch, int heads, float scale,
    const float *__restrict__ lse,
    const float *__restrict__ delta, T *__restrict__ dk, int64_t dk_stride, T *__restrict__ dv, int64_t dv_stride) {
  constexpr int NC = D / 16, ND = D / 32, W = kAttnBwdWalk;
  constexpr int LDN = D + AttnT<T>::PADN, LDT = W + AttnT<T>::PADT;
  extern __shared__ __attribute__((aligned(16))) unsigned char s_attn[];
  T *s_q = reinterpret_cast<T *>(s_attn);   // [W][LDN]
  T *s_g = s_q + W * LDN;                   // [W][LDN]   dO
  T *s_qt = s_g + W * LDN;                  // [D][LDT]
  T *s_gt = s_qt + D * LDT;                 // [D][LDT]
  float *s_lse = reinterpret_cast<float *>(s_gt + D * LDT);   // [W]
  float *s_delta = s_lse + W;                                 // [W]
  int b, t0, startk, lenk;
  if (!attn_find_item(blk_tab, seg_ptr_kv, n_batch, blockIdx.x, kAttnBlock, b, t0, startk, lenk)) return;
  const int head = blockIdx.y;
  const int startq = seg_ptr_q[b], lenq = seg_ptr_q[b + 1] - startq;
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, r = lane & 31, h = lane >> 5;
  const int tk = t0 + wave * 32 + r;
  const bool validk = tk < lenk, wave_on = t0 + wave * 32 < lenk;
  const int64_t ki = seg_rows_kv[startk + min(tk, lenk - 1)];
  AttnFrag<T> kf[NC], vf[NC];
  {
    const T *kp = k + ki * k_stride + (int64_t)head * D + 8 * h;
    const T *vp = v + ki * v_stride + (int64_t)head * D + 8 * h;
#pragma unroll
    for (int c = 0; c < NC; ++c) {
      kf[c] = attn_load8(kp + 16 * c);
      vf[c] = attn_load8(vp + 16 * c);
    }
  }
  at_f32x16 ak[ND], av[ND];
#pragma unroll
  for (int dt = 0; dt < ND; ++dt)
#pragma unroll
    for (int i = 0; i < 16; ++i) { ak[dt][i] = 0.f; av[dt][i] = 0.f; }
  const bool want_k = dk != nullptr, want_v = dv != nullptr;
  for (int q0 = 0; q0 < lenq; q0 += W) {
    __syncthreads();
    attn_stage<T, D, W>(q, q_stride, head, seg_rows_q, startq, lenq, q0, s_q, false, s_qt);
    attn_stage<T, D, W>(dout, dout_stride, head, seg_rows_q, startq, lenq, q0, s_g, true, s_gt);
    if (threadIdx.x < W) {
      const int w = threadIdx.x;
      const bool valid = q0 + w < lenq;
      const int64_t row = seg_rows_q[startq + min(q0 + w, lenq - 1)];
      s_lse[w] = lse[row * heads + head];
      s_delta[w] = valid ? delta[row * heads + head] : 0.f;
    }
    __syncthreads();
    if (!wave_on) continue;
    at_f32x16 s, dp;
#pragma unroll
    for (int i = 0; i < 16; ++i) { s[i] = 0.f; dp[i] = 0.f; }
    const T *qp = s_q + r * LDN + 8 * h, *gp = s_g + r * LDN + 8 * h;
#pragma unroll
    for (int c = 0; c < NC; ++c) attn_mma(s, attn_load8(qp + 16 * c), kf[c]);   // S[query][key]
    if (want_k) {
#pragma unroll
      for (int c = 0; c < NC; ++c) attn_mma(dp, attn_load8(gp + 16 * c), vf[c]);   // dP[query][key]
    }
    float p[16], ds[16];
#pragma unroll
    for (int i = 0; i < 16; ++i) {
      const int w = attn_row(i, h);
      p[i] = (q0 + w < lenq) ? attn_exp<T>(s[i] * scale - s_lse[w]) : 0.f;
      ds[i] = p[i] * (dp[i] - s_delta[w]);
    }
#pragma unroll
    for (int s2 = 0; s2 < 2; ++s2) {
      if (want_v) {
        const AttnFrag<T> pf = attn_acc_frag<T>(p, s2);
#pragma unroll
        for (int dt = 0; dt < ND; ++dt)   // dV^T[channel][key] += dO^T[channel][query] P[query][key]
          attn_mma(av[dt], attn_load44(s_gt + (dt * 32 + r) * LDT + 16 * s2 + 4 * h), pf);
      }
      if (want_k) {
        const AttnFrag<T> df = attn_acc_frag<T>(ds, s2);
#pragma unroll
        for (int dt = 0; dt < ND; ++dt)   // dK^T[channel][key] += Q^T[channel][query] dS[query][key]
          attn_mma(ak[dt], attn_load44(s_qt + (dt * 32 + r) * LDT + 16 * s2 + 4 * h), df);
      }
    }
  }
  if (!validk) return;
  if (want_k) attn_store_rows<T, D>(dk, dk_stride, ki, head, ak, scale, h);
  if (want_v) attn_store_rows<T, D>(dv, dv_stride, ki, head, av, 1.f, h);
}

// ---- backward: dK / dV split over the queries ------------------------------------------------------------------------
// With few keys and many queries (cross-attention to a short context) the key-stationary grid is a handful of workgroups
// that each walk every query of their instance.  k_attn_bwd_kv_split adds a grid dimension of S query slices: slice s of
// an instance of nblk = ceil(len_q / 32) query blocks walks the blocks [floor(s nblk / S), floor((s + 1) nblk / S)) and
// writes its unscaled fp32 partial of dK^T / dV^T (only the wanted ones; zeros from an empty slice) to row `key row` of
// image s of part_k / part_v [S][n_kv][c].  The workgroups of slice 0, head 0 also mark their key rows in `listed`
// (zeroed beforehand).  k_attn_kv_reduce then sums the S partials of every (key row, 4 channels) in ascending s, scales
// dK, rounds once and writes the gradient row; a row that no list holds gets zeros.  No atomics: bitwise reproducible.
// The walk repeats k_attn_bwd_kv's over a range of query blocks; that kernel keeps its text, and so its code object, for
// kv_splits = 1 (sharing the walk through an inlined function changed its register allocation).
template <typename T, int D>
__global__ __launch_bounds__(kAttnThreads) void k_attn_bwd_kv_split(
    const T *__restrict__ q, const T *__restrict__ k, const T *__restrict__ v, const T *__restrict__ dout,
    int64_t q_stride, int64_t k_stride, int64_t v_stride, int64_t dout_stride, const int32_t *__restrict__ seg_ptr_q,
    const int32_t *__restrict__ seg_rows_q, const int32_t *__restrict__ seg_ptr_kv,
    const int32_t *__restrict__ seg_rows_kv, const int32_t *__restrict__ blk_tab, int n_batch, int heads, float scale,
    const float *__restrict__ lse, const float *__restrict__ delta, int64_t n_kv, float *__restrict__ part_k,
    float *__restrict__ part_v, int32_t *__restrict__ listed) {
  int b, t0, startk, lenk;
  if (!attn_find_item(blk_tab, seg_ptr_kv, n_batch, blockIdx.x, kAttnBlock, b, t0, startk, lenk)) return;
  const int head = blockIdx.y;
  const int startq = seg_ptr_q[b], lenq = seg_ptr_q[b + 1] - startq;
  const int64_t nblk = (lenq + kAttnBwdWalk - 1) / kAttnBwdWalk, slice = blockIdx.z, n_slices = gridDim.z;
  const int q_lo = (int)(slice * nblk / n_slices) * kAttnBwdWalk, q_hi = (int)((slice + 1) * nblk / n_slices) * kAttnBwdWalk;
  const bool want_k = part_k != nullptr, want_v = part_v != nullptr;
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, r = lane & 31, h = lane >> 5;
  at_f32x16 ak[D / 32], av[D / 32];
  constexpr int NC = D / 16, ND = D / 32, W = kAttnBwdWalk;
  constexpr int LDN = D + AttnT<T>::PADN, LDT = W + AttnT<T>::PADT;
  extern __shared__ __attribute__((aligned(16))) unsigned char s_attn[];
  T *s_q = reinterpret_cast<T *>(s_attn);   // [W][LDN]
  T *s_g = s_q + W * LDN;                   // [W][LDN]   dO
  T *s_qt = s_g + W * LDN;                  // [D][LDT]
  T *s_gt = s_qt + D * LDT;                 // [D][LDT]
  float *s_lse = reinterpret_cast<float *>(s_gt + D * LDT);   // [W]
  float *s_delta = s_lse + W;                                 // [W]
  const int tk = t0 + wave * 32 + r;
  const bool validk = tk < lenk, wave_on = t0 + wave * 32 < lenk;
  const int64_t ki = seg_rows_kv[startk + min(tk, lenk - 1)];
  AttnFrag<T> kf[NC], vf[NC];
  {
    const T *kp = k + ki * k_stride + (int64_t)head * D + 8 * h;
    const T *vp = v + ki * v_stride + (int64_t)head * D + 8 * h;
#pragma unroll
    for (int c = 0; c < NC; ++c) {
      kf[c] = attn_load8(kp + 16 * c);
      vf[c] = attn_load8(vp + 16 * c);
    }
  }
#pragma unroll
  for (int dt = 0; dt < ND; ++dt)
#pragma unroll
    for (int i = 0; i < 16; ++i) { ak[dt][i] = 0.f; av[dt][i] = 0.f; }
  for (int q0 = q_lo; q0 < q_hi; q0 += W) {
    __syncthreads();
    attn_stage<T, D, W>(q, q_stride, head, seg_rows_q, startq, lenq, q0, s_q, false, s_qt);
    attn_stage<T, D, W>(dout, dout_stride, head, seg_rows_q, startq, lenq, q0, s_g, true, s_gt);
    if (threadIdx.x < W) {
      const int w = threadIdx.x;
      const bool valid = q0 + w < lenq;
      const int64_t row = seg_rows_q[startq + min(q0 + w, lenq - 1)];
      s_lse[w] = lse[row * heads + head];
      s_delta[w] = valid ? delta[row * heads + head] : 0.f;
    }
    __syncthreads();
    if (!wave_on) continue;
    at_f32x16 s, dp;
#pragma unroll
    for (int i = 0; i < 16; ++i) { s[i] = 0.f; dp[i] = 0.f; }
    const T *qp = s_q + r * LDN + 8 * h, *gp = s_g + r * LDN + 8 * h;
#pragma unroll
    for (int c = 0; c < NC; ++c) attn_mma(s, attn_load8(qp + 16 * c), kf[c]);   // S[query][key]
    if (want_k) {
#pragma unroll
      for (int c = 0; c < NC; ++c) attn_mma(dp, attn_load8(gp + 16 * c), vf[c]);   // dP[query][key]
    }
    float p[16], ds[16];
#pragma unroll
    for (int i = 0; i < 16; ++i) {
      const int w = attn_row(i, h);
      p[i] = (q0 + w < lenq) ? attn_exp<T>(s[i] * scale - s_lse[w]) : 0.f;
      ds[i] = p[i] * (dp[i] - s_delta[w]);
    }
#pragma unroll
    for (int s2 = 0; s2 < 2; ++s2) {
      if (want_v) {
        const AttnFrag<T> pf = attn_acc_frag<T>(p, s2);
#pragma unroll
        for (int dt = 0; dt < ND; ++dt)   // dV^T[channel][key] += dO^T[channel][query] P[query][key]
          attn_mma(av[dt], attn_load44(s_gt + (dt * 32 + r) * LDT + 16 * s2 + 4 * h), pf);
      }
      if (want_k) {
        const AttnFrag<T> df = attn_acc_frag<T>(ds, s2);
#pragma unroll
        for (int dt = 0; dt < ND; ++dt)   // dK^T[channel][key] += Q^T[channel][query] dS[query][key]
          attn_mma(ak[dt], attn_load44(s_qt + (dt * 32 + r) * LDT + 16 * s2 + 4 * h), df);
      }
    }
  }
  if (!validk) return;
  const int64_t c = (int64_t)heads * D, image = slice * n_kv * c;
  if (want_k) attn_store_rows<float, D>(part_k + image, c, ki, head, ak, 1.f, h);
  if (want_v) attn_store_rows<float, D>(part_v + image, c, ki, head, av, 1.f, h);
  if (slice == 0 && head == 0 && h == 0) listed[ki] = 1;
}

// thread: (key row, 4 channels) of the gradient blockIdx.y (0 dK, 1 dV)
template <typename T>
__global__ __launch_bounds__(256) void k_attn_kv_reduce(const float *__restrict__ part_k, const float *__restrict__ part_v,
                                                        const int32_t *__restrict__ listed, int64_t n_kv, int c,
                                                        int n_slices, float scale, T *__restrict__ dk, int64_t dk_stride,
                                                        T *__restrict__ dv, int64_t dv_stride) {
  const bool is_k = blockIdx.y == 0;
  const float *part = is_k ? part_k : part_v;
  T *y = is_k ? dk : dv;
  if (y == nullptr) return;
  const int pieces = c / 4;
  const int64_t id = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (id >= n_kv * pieces) return;
  const int64_t row = id / pieces;
  const int col = (int)(id - row * pieces) * 4;
  at_f32x4 acc;
  acc[0] = acc[1] = acc[2] = acc[3] = 0.f;
  if (listed[row]) {
    const float *p = part + row * c + col;
    for (int s = 0; s < n_slices; ++s) acc += *reinterpret_cast<const at_f32x4 *>(p + (int64_t)s * n_kv * c);
  }
  const float mul = is_k ? scale : 1.f;
  attn_store4(y + row * (is_k ? dk_stride : dv_stride) + col, acc[0] * mul, acc[1] * mul, acc[2] * mul, acc[3] * mul);
}

// ---- row lists of a dense context [n_batch, tokens, c]: segment b = rows b tokens + t, t < len_b ------------------------
// Thread i < n_batch * tokens places row i; thread i <= n_batch writes seg_ptr[i]; thread i < ceil(n_batch tokens / 64) +
// n_batch writes pair i of the block table.  Each sums the clamped lengths before its instance itself: O(n_batch) loads,
// a context batch being a handful of instances.  seg_rows past seg_ptr[n_batch] is not written.
__device__ __forceinline__ int attn_context_len(const int32_t *__restrict__ lengths, int b, int tokens) {
  return lengths ? min(max(lengths[b], 0), tokens) : tokens;
}
__global__ __launch_bounds__(256) void k_attn_context_lists(int n_batch, int tokens, const int32_t *__restrict__ lengths,
                                                           int64_t n_entries, int32_t *__restrict__ seg_ptr,
                                                           int32_t *__restrict__ seg_rows, int32_t *__restrict__ blk_tab) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < (int64_t)n_batch * tokens) {
    const int b = (int)(i / tokens), t = (int)(i - (int64_t)b * tokens);
    if (t < attn_context_len(lengths, b, tokens)) {
      int start = 0;
      for (int j = 0; j < b; ++j) start += attn_context_len(lengths, j, tokens);
      seg_rows[start + t] = (int32_t)i;
    }
  }
  if (i <= n_batch) {
    int start = 0;
    for (int j = 0; j < i; ++j) start += attn_context_len(lengths, j, tokens);
    seg_ptr[i] = start;
  }
  if (i < n_entries) {
    int seg = -1, first = -1, acc = 0;
    for (int b = 0; b < n_batch && seg < 0; ++b) {
      const int nb = (attn_context_len(lengths, b, tokens) + kAttnBlock - 1) / kAttnBlock;
      if (i < acc + nb) { seg = b; first = (int)(i - acc) * kAttnBlock; }
      acc += nb;
    }
    blk_tab[2 * i] = seg;
    blk_tab[2 * i + 1] = first;
  }
}

template <typename T, int D> constexpr int attn_fwd_lds() {
  return (int)sizeof(T) * (kAttnFwdWalk * (D + AttnT<T>::PADN) + D * (kAttnFwdWalk + AttnT<T>::PADT));
}
template <typename T, int D> constexpr int attn_bwd_q_lds() {
  return (int)sizeof(T) * (2 * kAttnBwdWalk * (D + AttnT<T>::PADN) + D * (kAttnBwdWalk + AttnT<T>::PADT));
}
template <typename T, int D> constexpr int attn_bwd_kv_lds() {
  return (int)sizeof(T) * (2 * kAttnBwdWalk * (D + AttnT<T>::PADN) + 2 * D * (kAttnBwdWalk + AttnT<T>::PADT)) +
         2 * kAttnBwdWalk * (int)sizeof(float);
}

struct AttnArgs {
  const void *q, *k, *v, *out, *dout;
  int64_t q_stride, k_stride, v_stride, out_stride, dout_stride, dq_stride, dk_stride, dv_stride;
  const int32_t *seg_ptr_q, *seg_rows_q, *seg_ptr_kv, *seg_rows_kv;
  const int32_t *tab_q, *tab_kv;   // block tables of the q / kv lists (null: the workgroups walk seg_ptr)
  int64_t n_q, n_kv;
  int n_batch, heads;
  float scale;
  void *out_w, *dq, *dk, *dv;
  float *lse, *delta;
  int kv_splits;                   // > 1: dK / dV through k_attn_bwd_kv_split and k_attn_kv_reduce
  float *part_k, *part_v;          // [kv_splits][n_kv][c] each
  int32_t *listed;                 // [n_kv]
};

// more than 48 KiB of dynamic LDS has to be allowed per kernel, once
#define ME_ATTN_LDS_ATTR(kernel, lds)                                                                                  \
  do {                                                                                                                 \
    static bool attr_set = false;                                                                                      \
    if ((lds) > 48 * 1024 && !attr_set) {                                                                              \
      ME_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(&kernel), hipFuncAttributeMaxDynamicSharedMemorySize,  \
                                 160 * 1024));                                                                         \
      attr_set = true;                                                                                                 \
    }                                                                                                                  \
  } while (0)

template <typename T, int D>
static int attn_forward_t(const AttnArgs &a, hipStream_t stream) {
  const dim3 grid((unsigned)(ceil_div(a.n_q, kAttnBlock) + a.n_batch), (unsigned)a.heads);
  ME_ATTN_LDS_ATTR((k_attn_fwd<T, D>), (attn_fwd_lds<T, D>()));
  k_attn_fwd<T, D><<<grid, kAttnThreads, attn_fwd_lds<T, D>(), stream>>>(
      (const T *)a.q, (const T *)a.k, (const T *)a.v, a.q_stride, a.k_stride, a.v_stride, a.seg_ptr_q, a.seg_rows_q,
      a.seg_ptr_kv, a.seg_rows_kv, a.tab_q, a.n_batch, a.heads, a.scale, (T *)a.out_w, a.out_stride, a.lse);
  ME_LAUNCH_CHECK();
  return 0;
}

template <typename T, int D>
static int attn_backward_t(const AttnArgs &a, hipStream_t stream) {
  {
    const dim3 grid((unsigned)ceil_div(a.n_q, 32), (unsigned)a.heads);
    k_attn_delta<T, D><<<grid, 64, 0, stream>>>((const T *)a.out, (const T *)a.dout, a.out_stride, a.dout_stride, a.n_q,
                                               a.heads, a.delta);
    ME_LAUNCH_CHECK();
  }
  if ((a.dk || a.dv) && a.n_kv > 0 && a.kv_splits > 1) {
    const dim3 grid((unsigned)(ceil_div(a.n_kv, kAttnBlock) + a.n_batch), (unsigned)a.heads, (unsigned)a.kv_splits);
    const int c = a.heads * D;
    ME_HIP(hipMemsetAsync(a.listed, 0, (size_t)a.n_kv * sizeof(int32_t), stream));
    ME_ATTN_LDS_ATTR((k_attn_bwd_kv_split<T, D>), (attn_bwd_kv_lds<T, D>()));
    k_attn_bwd_kv_split<T, D><<<grid, kAttnThreads, attn_bwd_kv_lds<T, D>(), stream>>>(
        (const T *)a.q, (const T *)a.k, (const T *)a.v, (const T *)a.dout, a.q_stride, a.k_stride, a.v_stride,
        a.dout_stride, a.seg_ptr_q, a.seg_rows_q, a.seg_ptr_kv, a.seg_rows_kv, a.tab_kv, a.n_batch, a.heads, a.scale, a.lse,
        a.delta, a.n_kv, a.dk ? a.part_k : nullptr, a.dv ? a.part_v : nullptr, a.listed);
    ME_LAUNCH_CHECK();
    const dim3 rgrid((unsigned)ceil_div(a.n_kv * (c / 4), 256), 2);
    k_attn_kv_reduce<T><<<rgrid, 256, 0, stream>>>(a.part_k, a.part_v, a.listed, a.n_kv, c, a.kv_splits, a.scale,
                                                   (T *)a.dk, a.dk_stride, (T *)a.dv, a.dv_stride);
    ME_LAUNCH_CHECK();
  } else if ((a.dk || a.dv) && a.n_kv > 0) {
    const dim3 grid((unsigned)(ceil_div(a.n_kv, kAttnBlock) + a.n_batch), (unsigned)a.heads);
    ME_ATTN_LDS_ATTR((k_attn_bwd_kv<T, D>), (attn_bwd_kv_lds<T, D>()));
    k_attn_bwd_kv<T, D><<<grid, kAttnThreads, attn_bwd_kv_lds<T, D>(), stream>>>(
        (const T *)a.q, (const T *)a.k, (const T *)a.v, (const T *)a.dout, a.q_stride, a.k_stride, a.v_stride,
        a.dout_stride, a.seg_ptr_q, a.seg_rows_q, a.seg_ptr_kv, a.seg_rows_kv, a.tab_kv, a.n_batch, a.heads, a.scale, a.lse,
        a.delta, (T *)a.dk, a.dk_stride, (T *)a.dv, a.dv_stride);
    ME_LAUNCH_CHECK();
  }
  if (a.dq) {
    const dim3 grid((unsigned)(ceil_div(a.n_q, kAttnBlock) + a.n_batch), (unsigned)a.heads);
    ME_ATTN_LDS_ATTR((k_attn_bwd_q<T, D>), (attn_bwd_q_lds<T, D>()));
    k_attn_bwd_q<T, D><<<grid, kAttnThreads, attn_bwd_q_lds<T, D>(), stream>>>(
        (const T *)a.q, (const T *)a.k, (const T *)a.v, (const T *)a.dout, a.q_stride, a.k_stride, a.v_stride,
        a.dout_stride, a.seg_ptr_q, a.seg_rows_q, a.seg_ptr_kv, a.seg_rows_kv, a.tab_q, a.n_batch, a.heads, a.scale, a.lse,
        a.delta, (T *)a.dq, a.dq_stride);
    ME_LAUNCH_CHECK();
  }
  return 0;
}

#define ME_ATTN_DISPATCH(is_bf16, d, fn, ...)                                                   \
  do {                                                                                          \
    if (is_bf16) {                                                                              \
      if ((d) == 32) return fn<__bf16, 32>(__VA_ARGS__);                                        \
      if ((d) == 64) return fn<__bf16, 64>(__VA_ARGS__);                                        \
      return fn<__bf16, 128>(__VA_ARGS__);                                                      \
    }                                                                                           \
    if ((d) == 32) return fn<float, 32>(__VA_ARGS__);                                           \
    if ((d) == 64) return fn<float, 64>(__VA_ARGS__);                                           \
    return fn<float, 128>(__VA_ARGS__);                                                         \
  } while (0)

// ---- float64 twins: plain double, one thread per (row of the list, head) ---------------------------------------------
__device__ __forceinline__ int attn_instance_of(const int32_t *__restrict__ seg_ptr, int n_batch, int64_t t) {
  int b = 0;
  while (b + 1 < n_batch && t >= seg_ptr[b + 1]) ++b;
  return b;
}

__global__ __launch_bounds__(256) void k_attn_fwd_f64(
    const double *__restrict__ q, const double *__restrict__ k, const double *__restrict__ v, int64_t q_stride,
    int64_t k_stride, int64_t v_stride, const int32_t *__restrict__ seg_ptr_q, const int32_t *__restrict__ seg_rows_q,
    const int32_t *__restrict__ seg_ptr_kv, const int32_t *__restrict__ seg_rows_kv, int64_t n_q, int n_batch, int heads,
    int d, double scale, double *__restrict__ out, int64_t out_stride, double *__restrict__ lse) {
  const int64_t id = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (id >= n_q * heads) return;
  const int64_t t = id / heads;
  if (t >= seg_ptr_q[n_batch]) return;   // a row that no list holds
  const int head = (int)(id - t * heads);
  const int b = attn_instance_of(seg_ptr_q, n_batch, t);
  const int64_t qi = seg_rows_q[t];
  const int k0 = seg_ptr_kv[b], k1 = seg_ptr_kv[b + 1];
  const double *qp = q + qi * q_stride + (int64_t)head * d;
  double *op = out + qi * out_stride + (int64_t)head * d;
  for (int c = 0; c < d; ++c) op[c] = 0.0;
  double m = -INFINITY;
  for (int j = k0; j < k1; ++j) {
    const double *kp = k + (int64_t)seg_rows_kv[j] * k_stride + (int64_t)head * d;
    double s = 0.0;
    for (int c = 0; c < d; ++c) s += qp[c] * kp[c];
    m = fmax(m, s * scale);
  }
  double l = 0.0;
  for (int j = k0; j < k1; ++j) {
    const double *kp = k + (int64_t)seg_rows_kv[j] * k_stride + (int64_t)head * d;
    const double *vp = v + (int64_t)seg_rows_kv[j] * v_stride + (int64_t)head * d;
    double s = 0.0;
    for (int c = 0; c < d; ++c) s += qp[c] * kp[c];
    const double p = exp(s * scale - m);
    l += p;
    for (int c = 0; c < d; ++c) op[c] += p * vp[c];
  }
  if (k1 > k0)
    for (int c = 0; c < d; ++c) op[c] /= l;
  lse[qi * heads + head] = k1 > k0 ? m + log(l) : -INFINITY;
}

__global__ __launch_bounds__(256) void k_attn_bwd_q_f64(
    const double *__restrict__ q, const double *__restrict__ k, const double *__restrict__ v,
    const double *__restrict__ out, const double *__restrict__ dout, int64_t q_stride, int64_t k_stride, int64_t v_stride,
    int64_t out_stride, int64_t dout_stride, const int32_t *__restrict__ seg_ptr_q, const int32_t *__restrict__ seg_rows_q,
    const int32_t *__restrict__ seg_ptr_kv, const int32_t *__restrict__ seg_rows_kv, int64_t n_q, int n_batch, int heads,
    int d, double scale, const double *__restrict__ lse, double *__restrict__ dq, int64_t dq_stride) {
  const int64_t id = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (id >= n_q * heads) return;
  const int64_t t = id / heads;
  if (t >= seg_ptr_q[n_batch]) return;   // a row that no list holds
  const int head = (int)(id - t * heads);
  const int b = attn_instance_of(seg_ptr_q, n_batch, t);
  const int64_t qi = seg_rows_q[t];
  const int k0 = seg_ptr_kv[b], k1 = seg_ptr_kv[b + 1];
  const double *qp = q + qi * q_stride + (int64_t)head * d;
  const double *op = out + qi * out_stride + (int64_t)head * d;
  const double *gp = dout + qi * dout_stride + (int64_t)head * d;
  double *dp = dq + qi * dq_stride + (int64_t)head * d;
  const double ls = lse[qi * heads + head];
  double delta = 0.0;
  for (int c = 0; c < d; ++c) {
    delta += gp[c] * op[c];
    dp[c] = 0.0;
  }
  for (int j = k0; j < k1; ++j) {
    const double *kp = k + (int64_t)seg_rows_kv[j] * k_stride + (int64_t)head * d;
    const double *vp = v + (int64_t)seg_rows_kv[j] * v_stride + (int64_t)head * d;
    double s = 0.0, dpv = 0.0;
    for (int c = 0; c < d; ++c) {
      s += qp[c] * kp[c];
      dpv += gp[c] * vp[c];
    }
    const double ds = exp(s * scale - ls) * (dpv - delta) * scale;
    for (int c = 0; c < d; ++c) dp[c] += ds * kp[c];
  }
}

__global__ __launch_bounds__(256) void k_attn_bwd_kv_f64(
    const double *__restrict__ q, const double *__restrict__ k, const double *__restrict__ v,
    const double *__restrict__ out, const double *__restrict__ dout, int64_t q_stride, int64_t k_stride, int64_t v_stride,
    int64_t out_stride, int64_t dout_stride, const int32_t *__restrict__ seg_ptr_q, const int32_t *__restrict__ seg_rows_q,
    const int32_t *__restrict__ seg_ptr_kv, const int32_t *__restrict__ seg_rows_kv, int64_t n_kv, int n_batch, int heads,
    int d, double scale, const double *__restrict__ lse, double *__restrict__ dk, int64_t dk_stride,
    double *__restrict__ dv, int64_t dv_stride) {
  const int64_t id = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (id >= n_kv * heads) return;
  const int64_t t = id / heads;
  if (t >= seg_ptr_kv[n_batch]) return;   // a row that no list holds
  const int head = (int)(id - t * heads);
  const int b = attn_instance_of(seg_ptr_kv, n_batch, t);
  const int64_t ki = seg_rows_kv[t];
  const int q0 = seg_ptr_q[b], q1 = seg_ptr_q[b + 1];
  const double *kp = k + ki * k_stride + (int64_t)head * d;
  const double *vp = v + ki * v_stride + (int64_t)head * d;
  double *dkp = dk ? dk + ki * dk_stride + (int64_t)head * d : nullptr;
  double *dvp = dv ? dv + ki * dv_stride + (int64_t)head * d : nullptr;
  for (int c = 0; c < d; ++c) {
    if (dkp) dkp[c] = 0.0;
    if (dvp) dvp[c] = 0.0;
  }
  for (int i = q0; i < q1; ++i) {
    const int64_t qi = seg_rows_q[i];
    const double *qp = q + qi * q_stride + (int64_t)head * d;
    const double *op = out + qi * out_stride + (int64_t)head * d;
    const double *gp = dout + qi * dout_stride + (int64_t)head * d;
    double s = 0.0, dpv = 0.0, delta = 0.0;
    for (int c = 0; c < d; ++c) {
      s += qp[c] * kp[c];
      dpv += gp[c] * vp[c];
      delta += gp[c] * op[c];
    }
    const double p = exp(s * scale - lse[qi * heads + head]);
    const double ds = p * (dpv - delta) * scale;
    for (int c = 0; c < d; ++c) {
      if (dvp) dvp[c] += p * gp[c];
      if (dkp) dkp[c] += ds * qp[c];
    }
  }
}

static bool attn_aligned16(const void *p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

}  // namespace me

using namespace me;

// the argument checks shared by the entry points; `unit`: elements of 16 bytes (0: float64, any stride >= c)
#define ME_ATTN_CHECK_DIMS(unit)                                                                                       \
  ME_CHECK(n_q >= 0 && n_kv >= 0 && n_batch >= 0 && n_q < (1ll << 31) && n_kv < (1ll << 31), "bad row or instance count"); \
  ME_CHECK(heads > 0 && heads <= 65535 && c > 0, "bad head or channel count");                                         \
  ME_CHECK(c % heads == 0, "the channel count must be a multiple of the head count");                                  \
  ME_CHECK((unit) == 0 || c / heads == 32 || c / heads == 64 || c / heads == 128,                                      \
           "the head dimension must be 32, 64 or 128 (any on the float64 entry points)")
#define ME_ATTN_CHECK_STRIDE(s, unit)                                                                                  \
  ME_CHECK((s) >= c && ((unit) == 0 || (s) % (unit) == 0), "a row stride must be >= the channel count and a multiple of 16 bytes")
#define ME_ATTN_CHECK_TABLES()                                                                                         \
  ME_CHECK(seg_ptr_q != nullptr && seg_rows_q != nullptr && seg_ptr_kv != nullptr && seg_rows_kv != nullptr,           \
           "missing row-list table pointer (seg_ptr / seg_rows of both maps)")

extern "C" {

int64_t me_attn_workspace_bytes(int64_t n_q, int64_t n_kv, int32_t n_batch, int32_t heads) {
  (void)n_kv;
  (void)n_batch;   // the workgroups find their blocks by walking seg_ptr: no block table
  return align_up((n_q > 0 ? n_q : 0) * (int64_t)(heads > 0 ? heads : 0) * (int64_t)sizeof(float), 256);   // delta [n_q, heads]
}

// The _tab entry points are the implementation: me_attn_forward / me_attn_backward (below) pass null tables.  A table holds
// ceil(n / 64) + n_batch int32 pairs (the grid of its side); blk_tab_kv is not read by the forward pass.
int me_attn_forward_tab(const void *q, const void *k, const void *v, int32_t is_bf16, int64_t q_stride, int64_t k_stride,
                        int64_t v_stride, const int32_t *seg_ptr_q, const int32_t *seg_rows_q, const int32_t *seg_ptr_kv,
                        const int32_t *seg_rows_kv, const int32_t *blk_tab_q, const int32_t *blk_tab_kv, int64_t n_q,
                        int64_t n_kv, int32_t n_batch, int32_t c, int32_t heads, float scale, void *out,
                        int64_t out_stride, float *lse, void *stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  const int unit = is_bf16 ? 8 : 4;
  ME_ATTN_CHECK_DIMS(unit);
  ME_ATTN_CHECK_STRIDE(q_stride, unit);
  ME_ATTN_CHECK_STRIDE(k_stride, unit);
  ME_ATTN_CHECK_STRIDE(v_stride, unit);
  ME_ATTN_CHECK_STRIDE(out_stride, unit);
  ME_ATTN_CHECK_TABLES();
  if (n_q == 0 || n_batch == 0) return 0;
  ME_CHECK(q != nullptr && out != nullptr && lse != nullptr && (n_kv == 0 || (k != nullptr && v != nullptr)),
           "null data pointer");
  ME_CHECK(attn_aligned16(q) && attn_aligned16(k) && attn_aligned16(v) && attn_aligned16(out),
           "q, k, v and out must be 16-byte aligned");
  AttnArgs a{};
  a.q = q; a.k = k; a.v = v;
  a.q_stride = q_stride; a.k_stride = k_stride; a.v_stride = v_stride; a.out_stride = out_stride;
  a.seg_ptr_q = seg_ptr_q; a.seg_rows_q = seg_rows_q; a.seg_ptr_kv = seg_ptr_kv; a.seg_rows_kv = seg_rows_kv;
  a.tab_q = blk_tab_q; a.tab_kv = blk_tab_kv;
  a.n_q = n_q; a.n_kv = n_kv; a.n_batch = n_batch; a.heads = heads; a.scale = scale;
  a.out_w = out; a.lse = lse;
  ME_ATTN_DISPATCH(is_bf16, c / heads, attn_forward_t, a, stream);
}

int me_attn_forward(const void *q, const void *k, const void *v, int32_t is_bf16, int64_t q_stride, int64_t k_stride,
                    int64_t v_stride, const int32_t *seg_ptr_q, const int32_t *seg_rows_q, const int32_t *seg_ptr_kv,
                    const int32_t *seg_rows_kv, int64_t n_q, int64_t n_kv, int32_t n_batch, int32_t c, int32_t heads,
                    float scale, void *out, int64_t out_stride, float *lse, void *stream_) {
  return me_attn_forward_tab(q, k, v, is_bf16, q_stride, k_stride, v_stride, seg_ptr_q, seg_rows_q, seg_ptr_kv, seg_rows_kv,
                             nullptr, nullptr, n_q, n_kv, n_batch, c, heads, scale, out, out_stride, lse, stream_);
}

// the workspace of me_attn_backward_split: delta, the marks of the listed key rows, the partial images of dK and dV
struct AttnSplitWs {
  int64_t listed, part_k, part_v, bytes;   // byte offsets
};
static AttnSplitWs attn_split_ws(int64_t n_q, int64_t n_kv, int32_t c, int32_t heads, int32_t kv_splits) {
  const int64_t nq = n_q > 0 ? n_q : 0, nk = n_kv > 0 ? n_kv : 0, ch = c > 0 ? c : 0, h = heads > 0 ? heads : 0;
  const int64_t image = align_up((kv_splits > 0 ? kv_splits : 0) * nk * ch * (int64_t)sizeof(float), 256);
  AttnSplitWs w;
  w.listed = align_up(nq * h * (int64_t)sizeof(float), 256);
  w.part_k = w.listed + align_up(nk * (int64_t)sizeof(int32_t), 256);
  w.part_v = w.part_k + image;
  w.bytes = w.part_v + image;
  return w;
}

int64_t me_attn_split_workspace_bytes(int64_t n_q, int64_t n_kv, int32_t n_batch, int32_t c, int32_t heads,
                                      int32_t kv_splits) {
  (void)n_batch;
  return attn_split_ws(n_q, n_kv, c, heads, kv_splits).bytes;
}

// The policy of the cross-attention operators: how many query slices the dK / dV pass takes.  A pure function of the
// shape.  The key-stationary grid has wgs = (ceil(n_kv / 64) + n_batch) * heads workgroups of two waves; at the one wave
// per SIMD the kernels reach for d >= 64 a CU holds two of them, the chip kAttnSplitSlots = 512.  S = floor(512 / wgs):
// the slices of all workgroups still run in ONE round, each walking 1 / S of the queries (a second round would give back
// what the shorter walk wins: measured).  So S = 1 as soon as wgs > 256 — every self-attention shape of
// scripts/attention_bench.py, where n_kv = n_q.  Bounded by ME_ATTN_MAX_KV_SPLITS, by kAttnSplitMinQueries queries of an
// average instance per slice (the shortest measured, 156, still won) and by kAttnSplitMaxBytes of partial images.
// Measurement: DESIGN 8.14.
constexpr int64_t kAttnSplitSlots = 512;
constexpr int64_t kAttnSplitMinQueries = 256;
constexpr int64_t kAttnSplitMaxBytes = 64ll << 20;
int32_t me_attn_kv_splits(int64_t n_q, int64_t n_kv, int32_t n_batch, int32_t c, int32_t heads) {
  if (n_q <= 0 || n_kv <= 0 || n_batch <= 0 || c <= 0 || heads <= 0) return 1;
  const int64_t wgs = (ceil_div(n_kv, kAttnBlock) + n_batch) * heads;
  int64_t s = kAttnSplitSlots / wgs;
  s = std::min<int64_t>(s, ME_ATTN_MAX_KV_SPLITS);
  s = std::min<int64_t>(s, n_q / n_batch / kAttnSplitMinQueries);
  s = std::min<int64_t>(s, kAttnSplitMaxBytes / (2 * n_kv * c * (int64_t)sizeof(float)));
  return (int32_t)std::max<int64_t>(s, 1);
}

// kv_splits 0: me_attn_backward_tab (the workspace holds delta only); >= 1: me_attn_backward_split
static int attn_backward_entry(const void *q, const void *k, const void *v, const void *out, const float *lse,
                               const void *dout, int32_t is_bf16, int64_t q_stride, int64_t k_stride, int64_t v_stride,
                               int64_t out_stride, int64_t dout_stride, const int32_t *seg_ptr_q,
                               const int32_t *seg_rows_q, const int32_t *seg_ptr_kv, const int32_t *seg_rows_kv,
                               const int32_t *blk_tab_q, const int32_t *blk_tab_kv, int64_t n_q, int64_t n_kv,
                               int32_t n_batch, int32_t c, int32_t heads, float scale, void *dq, int64_t dq_stride,
                               void *dk, int64_t dk_stride, void *dv, int64_t dv_stride, void *workspace,
                               int64_t workspace_bytes, int32_t kv_splits, void *stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  const int unit = is_bf16 ? 8 : 4;
  ME_ATTN_CHECK_DIMS(unit);
  ME_ATTN_CHECK_STRIDE(q_stride, unit);
  ME_ATTN_CHECK_STRIDE(k_stride, unit);
  ME_ATTN_CHECK_STRIDE(v_stride, unit);
  ME_ATTN_CHECK_STRIDE(out_stride, unit);
  ME_ATTN_CHECK_STRIDE(dout_stride, unit);
  ME_CHECK(dq == nullptr || (dq_stride >= c && dq_stride % unit == 0), "dq: a row stride must be >= the channel count and a multiple of 16 bytes");
  ME_CHECK(dk == nullptr || (dk_stride >= c && dk_stride % unit == 0), "dk: a row stride must be >= the channel count and a multiple of 16 bytes");
  ME_CHECK(dv == nullptr || (dv_stride >= c && dv_stride % unit == 0), "dv: a row stride must be >= the channel count and a multiple of 16 bytes");
  ME_CHECK(workspace_bytes >= (kv_splits == 0 ? me_attn_workspace_bytes(n_q, n_kv, n_batch, heads)
                                              : me_attn_split_workspace_bytes(n_q, n_kv, n_batch, c, heads, kv_splits)),
           "workspace too small");
  ME_ATTN_CHECK_TABLES();
  if (n_batch == 0 || (n_q == 0 && n_kv == 0)) return 0;
  if (dq == nullptr && dk == nullptr && dv == nullptr) return 0;
  if (n_q == 0) {   // keys without queries: zero gradients
    const size_t row = (size_t)c * (is_bf16 ? 2 : 4);
    if (dk) ME_HIP(hipMemset2DAsync(dk, (size_t)dk_stride * (is_bf16 ? 2 : 4), 0, row, (size_t)n_kv, stream));
    if (dv) ME_HIP(hipMemset2DAsync(dv, (size_t)dv_stride * (is_bf16 ? 2 : 4), 0, row, (size_t)n_kv, stream));
    return 0;
  }
  ME_CHECK(q != nullptr && out != nullptr && lse != nullptr && dout != nullptr && workspace != nullptr &&
               (n_kv == 0 || (k != nullptr && v != nullptr)),
           "null data pointer");
  ME_CHECK(attn_aligned16(q) && attn_aligned16(k) && attn_aligned16(v) && attn_aligned16(out) && attn_aligned16(dout) &&
               attn_aligned16(dq) && attn_aligned16(dk) && attn_aligned16(dv) && attn_aligned16(workspace),
           "q, k, v, out, dout, the gradients and the workspace must be 16-byte aligned");
  AttnArgs a{};
  a.q = q; a.k = k; a.v = v; a.out = out; a.dout = dout;
  a.q_stride = q_stride; a.k_stride = k_stride; a.v_stride = v_stride; a.out_stride = out_stride;
  a.dout_stride = dout_stride; a.dq_stride = dq_stride; a.dk_stride = dk_stride; a.dv_stride = dv_stride;
  a.seg_ptr_q = seg_ptr_q; a.seg_rows_q = seg_rows_q; a.seg_ptr_kv = seg_ptr_kv; a.seg_rows_kv = seg_rows_kv;
  a.n_q = n_q; a.n_kv = n_kv; a.n_batch = n_batch; a.heads = heads; a.scale = scale;
  a.dq = dq; a.dk = dk; a.dv = dv;
  a.lse = const_cast<float *>(lse);
  a.delta = reinterpret_cast<float *>(workspace);
  a.tab_q = blk_tab_q; a.tab_kv = blk_tab_kv;
  a.kv_splits = kv_splits;
  if (kv_splits > 1) {
    const AttnSplitWs w = attn_split_ws(n_q, n_kv, c, heads, kv_splits);
    char *base = reinterpret_cast<char *>(workspace);
    a.listed = reinterpret_cast<int32_t *>(base + w.listed);
    a.part_k = reinterpret_cast<float *>(base + w.part_k);
    a.part_v = reinterpret_cast<float *>(base + w.part_v);
  }
  ME_ATTN_DISPATCH(is_bf16, c / heads, attn_backward_t, a, stream);
}

int me_attn_backward_tab(const void *q, const void *k, const void *v, const void *out, const float *lse, const void *dout,
                         int32_t is_bf16, int64_t q_stride, int64_t k_stride, int64_t v_stride, int64_t out_stride,
                         int64_t dout_stride, const int32_t *seg_ptr_q, const int32_t *seg_rows_q,
                         const int32_t *seg_ptr_kv, const int32_t *seg_rows_kv, const int32_t *blk_tab_q,
                         const int32_t *blk_tab_kv, int64_t n_q, int64_t n_kv, int32_t n_batch, int32_t c, int32_t heads,
                         float scale, void *dq, int64_t dq_stride, void *dk, int64_t dk_stride, void *dv,
                         int64_t dv_stride, void *workspace, int64_t workspace_bytes, void *stream_) {
  return attn_backward_entry(q, k, v, out, lse, dout, is_bf16, q_stride, k_stride, v_stride, out_stride, dout_stride,
                             seg_ptr_q, seg_rows_q, seg_ptr_kv, seg_rows_kv, blk_tab_q, blk_tab_kv, n_q, n_kv, n_batch, c,
                             heads, scale, dq, dq_stride, dk, dk_stride, dv, dv_stride, workspace, workspace_bytes, 0,
                             stream_);
}

// me_attn_backward_tab with the dK / dV pass cut into kv_splits query slices (1: the same launches, bit for bit)
int me_attn_backward_split(const void *q, const void *k, const void *v, const void *out, const float *lse,
                           const void *dout, int32_t is_bf16, int64_t q_stride, int64_t k_stride, int64_t v_stride,
                           int64_t out_stride, int64_t dout_stride, const int32_t *seg_ptr_q, const int32_t *seg_rows_q,
                           const int32_t *seg_ptr_kv, const int32_t *seg_rows_kv, const int32_t *blk_tab_q,
                           const int32_t *blk_tab_kv, int64_t n_q, int64_t n_kv, int32_t n_batch, int32_t c,
                           int32_t heads, float scale, void *dq, int64_t dq_stride, void *dk, int64_t dk_stride, void *dv,
                           int64_t dv_stride, void *workspace, int64_t workspace_bytes, int32_t kv_splits, void *stream_) {
  ME_CHECK(kv_splits >= 1 && kv_splits <= ME_ATTN_MAX_KV_SPLITS, "kv_splits must be between 1 and ME_ATTN_MAX_KV_SPLITS (32)");
  return attn_backward_entry(q, k, v, out, lse, dout, is_bf16, q_stride, k_stride, v_stride, out_stride, dout_stride,
                             seg_ptr_q, seg_rows_q, seg_ptr_kv, seg_rows_kv, blk_tab_q, blk_tab_kv, n_q, n_kv, n_batch, c,
                             heads, scale, dq, dq_stride, dk, dk_stride, dv, dv_stride, workspace, workspace_bytes,
                             kv_splits, stream_);
}

// the row lists and block table of a dense context of n_batch x tokens rows (k_attn_context_lists): one launch
int me_attn_context_lists(int32_t n_batch, int32_t tokens, const int32_t *lengths, int32_t *seg_ptr, int32_t *seg_rows,
                          int32_t *blk_tab, void *stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  ME_CHECK(n_batch >= 0, "n_batch must not be negative");
  ME_CHECK(tokens >= 1, "tokens must be at least 1");
  const int64_t n = (int64_t)n_batch * tokens;
  ME_CHECK(n < (1ll << 31), "the context rows must fit in int32");
  ME_CHECK(seg_ptr != nullptr && blk_tab != nullptr && (n_batch == 0 || seg_rows != nullptr),
           "seg_ptr, seg_rows and blk_tab must be given");
  const int64_t n_entries = ceil_div(n, kAttnBlock) + n_batch;
  const int64_t threads = std::max<int64_t>(std::max<int64_t>(n, n_entries), n_batch + 1);
  k_attn_context_lists<<<(unsigned)ceil_div(threads, 256), 256, 0, stream>>>(n_batch, tokens, lengths, n_entries, seg_ptr,
                                                                             seg_rows, blk_tab);
  ME_LAUNCH_CHECK();
  return 0;
}

int me_attn_backward(const void *q, const void *k, const void *v, const void *out, const float *lse, const void *dout,
                     int32_t is_bf16, int64_t q_stride, int64_t k_stride, int64_t v_stride, int64_t out_stride,
                     int64_t dout_stride, const int32_t *seg_ptr_q, const int32_t *seg_rows_q, const int32_t *seg_ptr_kv,
                     const int32_t *seg_rows_kv, int64_t n_q, int64_t n_kv, int32_t n_batch, int32_t c, int32_t heads,
                     float scale, void *dq, int64_t dq_stride, void *dk, int64_t dk_stride, void *dv, int64_t dv_stride,
                     void *workspace, int64_t workspace_bytes, void *stream_) {
  return me_attn_backward_tab(q, k, v, out, lse, dout, is_bf16, q_stride, k_stride, v_stride, out_stride, dout_stride,
                              seg_ptr_q, seg_rows_q, seg_ptr_kv, seg_rows_kv, nullptr, nullptr, n_q, n_kv, n_batch, c, heads,
                              scale, dq, dq_stride, dk, dk_stride, dv, dv_stride, workspace, workspace_bytes, stream_);
}

int me_attn_forward_f64(const double *q, const double *k, const double *v, int64_t q_stride, int64_t k_stride,
                        int64_t v_stride, const int32_t *seg_ptr_q, const int32_t *seg_rows_q, const int32_t *seg_ptr_kv,
                        const int32_t *seg_rows_kv, int64_t n_q, int64_t n_kv, int32_t n_batch, int32_t c, int32_t heads,
                        double scale, double *out, int64_t out_stride, double *lse, void *stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  ME_ATTN_CHECK_DIMS(0);
  ME_ATTN_CHECK_STRIDE(q_stride, 0);
  ME_ATTN_CHECK_STRIDE(k_stride, 0);
  ME_ATTN_CHECK_STRIDE(v_stride, 0);
  ME_ATTN_CHECK_STRIDE(out_stride, 0);
  ME_ATTN_CHECK_TABLES();
  if (n_q == 0 || n_batch == 0) return 0;
  ME_CHECK(q != nullptr && out != nullptr && lse != nullptr && (n_kv == 0 || (k != nullptr && v != nullptr)),
           "null data pointer");
  const int64_t items = n_q * heads;
  k_attn_fwd_f64<<<(unsigned)ceil_div(items, 256), 256, 0, stream>>>(q, k, v, q_stride, k_stride, v_stride, seg_ptr_q,
                                                                    seg_rows_q, seg_ptr_kv, seg_rows_kv, n_q, n_batch,
                                                                    heads, c / heads, scale, out, out_stride, lse);
  ME_LAUNCH_CHECK();
  return 0;
}

int me_attn_backward_f64(const double *q, const double *k, const double *v, const double *out, const double *lse,
                         const double *dout, int64_t q_stride, int64_t k_stride, int64_t v_stride, int64_t out_stride,
                         int64_t dout_stride, const int32_t *seg_ptr_q, const int32_t *seg_rows_q,
                         const int32_t *seg_ptr_kv, const int32_t *seg_rows_kv, int64_t n_q, int64_t n_kv, int32_t n_batch,
                         int32_t c, int32_t heads, double scale, double *dq, int64_t dq_stride, double *dk,
                         int64_t dk_stride, double *dv, int64_t dv_stride, void *stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  ME_ATTN_CHECK_DIMS(0);
  ME_ATTN_CHECK_STRIDE(q_stride, 0);
  ME_ATTN_CHECK_STRIDE(k_stride, 0);
  ME_ATTN_CHECK_STRIDE(v_stride, 0);
  ME_ATTN_CHECK_STRIDE(out_stride, 0);
  ME_ATTN_CHECK_STRIDE(dout_stride, 0);
  ME_CHECK((dq == nullptr || dq_stride >= c) && (dk == nullptr || dk_stride >= c) && (dv == nullptr || dv_stride >= c),
           "a gradient row stride must be >= the channel count");
  ME_ATTN_CHECK_TABLES();
  if (n_batch == 0) return 0;
  ME_CHECK((n_q == 0 || (q != nullptr && out != nullptr && lse != nullptr && dout != nullptr)) &&
               (n_kv == 0 || (k != nullptr && v != nullptr)),
           "null data pointer");
  if ((dk || dv) && n_kv > 0) {
    k_attn_bwd_kv_f64<<<(unsigned)ceil_div(n_kv * heads, 256), 256, 0, stream>>>(
        q, k, v, out, dout, q_stride, k_stride, v_stride, out_stride, dout_stride, seg_ptr_q, seg_rows_q, seg_ptr_kv,
        seg_rows_kv, n_kv, n_batch, heads, c / heads, scale, lse, dk, dk_stride, dv, dv_stride);
    ME_LAUNCH_CHECK();
  }
  if (dq && n_q > 0) {
    k_attn_bwd_q_f64<<<(unsigned)ceil_div(n_q * heads, 256), 256, 0, stream>>>(
        q, k, v, out, dout, q_stride, k_stride, v_stride, out_stride, dout_stride, seg_ptr_q, seg_rows_q, seg_ptr_kv,
        seg_rows_kv, n_q, n_batch, heads, c / heads, scale, lse, dq, dq_stride);
    ME_LAUNCH_CHECK();
  }
  return 0;
}

// The float64 twins take the tables for a uniform call and do not read them: a thread finds its segment from seg_ptr.
int me_attn_forward_tab_f64(const double *q, const double *k, const double *v, int64_t q_stride, int64_t k_stride,
                            int64_t v_stride, const int32_t *seg_ptr_q, const int32_t *seg_rows_q,
                            const int32_t *seg_ptr_kv, const int32_t *seg_rows_kv, const int32_t *blk_tab_q,
                            const int32_t *blk_tab_kv, int64_t n_q, int64_t n_kv, int32_t n_batch, int32_t c,
                            int32_t heads, double scale, double *out, int64_t out_stride, double *lse, void *stream_) {
  (void)blk_tab_q;
  (void)blk_tab_kv;
  return me_attn_forward_f64(q, k, v, q_stride, k_stride, v_stride, seg_ptr_q, seg_rows_q, seg_ptr_kv, seg_rows_kv, n_q,
                             n_kv, n_batch, c, heads, scale, out, out_stride, lse, stream_);
}

int me_attn_backward_tab_f64(const double *q, const double *k, const double *v, const double *out, const double *lse,
                             const double *dout, int64_t q_stride, int64_t k_stride, int64_t v_stride, int64_t out_stride,
                             int64_t dout_stride, const int32_t *seg_ptr_q, const int32_t *seg_rows_q,
                             const int32_t *seg_ptr_kv, const int32_t *seg_rows_kv, const int32_t *blk_tab_q,
                             const int32_t *blk_tab_kv, int64_t n_q, int64_t n_kv, int32_t n_batch, int32_t c,
                             int32_t heads, double scale, double *dq, int64_t dq_stride, double *dk, int64_t dk_stride,
                             double *dv, int64_t dv_stride, void *stream_) {
  (void)blk_tab_q;
  (void)blk_tab_kv;
  return me_attn_backward_f64(q, k, v, out, lse, dout, q_stride, k_stride, v_stride, out_stride, dout_stride, seg_ptr_q,
                              seg_rows_q, seg_ptr_kv, seg_rows_kv, n_q, n_kv, n_batch, c, heads, scale, dq, dq_stride, dk,
                              dk_stride, dv, dv_stride, stream_);
}

int me_attn_backward_split_f64(const double *q, const double *k, const double *v, const double *out, const double *lse,
                               const double *dout, int64_t q_stride, int64_t k_stride, int64_t v_stride,
                               int64_t out_stride, int64_t dout_stride, const int32_t *seg_ptr_q,
                               const int32_t *seg_rows_q, const int32_t *seg_ptr_kv, const int32_t *seg_rows_kv,
                               const int32_t *blk_tab_q, const int32_t *blk_tab_kv, int64_t n_q, int64_t n_kv,
                               int32_t n_batch, int32_t c, int32_t heads, double scale, double *dq, int64_t dq_stride,
                               double *dk, int64_t dk_stride, double *dv, int64_t dv_stride, int32_t kv_splits,
                               void *stream_) {
  (void)blk_tab_q;
  (void)blk_tab_kv;
  (void)kv_splits;
  return me_attn_backward_f64(q, k, v, out, lse, dout, q_stride, k_stride, v_stride, out_stride, dout_stride, seg_ptr_q,
                              seg_rows_q, seg_ptr_kv, seg_rows_kv, n_q, n_kv, n_batch, c, heads, scale, dq, dq_stride, dk,
                              dk_stride, dv, dv_stride, stream_);
}

}  // extern "C"
