// Mamba-2 state-space-dual scan (SSD) over the serialized voxel order, for gfx950 (MI355X): MinkowskiMamba2,
// MinkowskiFunctional.ssd_scan (ABI 1.29).  The sequence is the selective scan's (selective_scan.hip): position p is row
// seg_rows[p] (seg_rows[n - 1 - p] with `reverse`), and a position whose row belongs to another instance than the position
// before it (and position 0) starts from a zero state.  H heads of width P, S states, G groups; head h reads group
// h / (H / G) of B and C:
//   dt  = dt_in[row, h] + dt_bias[h]                                  (softplus of that, torch's threshold form, when asked)
//   h_t = exp(dt A[h]) h_{t-1} + dt B[row, g, :] (outer) x[row, h, :]                                  an S x P state a head
//   y[row, h, :] = C[row, g, :] . h_t + D[h] x[row, h, :]
// A is one scalar a head, so inside a chunk of kT = 64 positions the recurrence is three matrix products and between the
// chunks one scalar-times-state carry.  With a_t = dt_t A, cum_i = sum_{t <= i} a_t over the chunk (a plain sum that ignores
// the starts, in fp64: only DIFFERENCES of it reach an exponential) and seg_i = the starts at positions <= i:
//   L_ij  = exp(cum_i - cum_j)        where j <= i and seg_i = seg_j, else 0          (never a -inf in a log-space sum)
//   e_i   = exp(cum_i)                where seg_i = 0, else 0                          (what position i sees of the entry state)
//   f_j   = exp(cum_last - cum_j)     where seg_j = seg_last, else 0                   (what the end state sees of position j)
//   decay = exp(cum_last)             where seg_last = 0, else 0
//   Y = ((C B^T) o L) diag(dt) X + diag(e) C entry + D X,        end = B^T diag(f dt) X,        entry' = decay entry + end
//
// Products.  Every product is v_mfma_f32_32x32x16_bf16 (bf16 rows: operands rounded to bf16, the decay-weighted ones too) or
// the exact v_mfma_f32_32x32x2_f32 (fp32 rows) with fp32 accumulation, on operands that the four waves of a workgroup read
// from the chunk's LDS images (B, C, X, dY and two 64 x 64 tiles in the rows' type) or, for the S x P states, straight from
// memory in fp32.  mma_seg() adds one (A, B, K) segment to a 32 x 32 accumulator tile of a wave; a product with two
// sources is two segments into two accumulators that the epilogue combines in fp32.  The one exception is mma_seg64 in
// k_ssd_bwd on fp32 rows.
//   forward   k_ssd_state<.., false>  (chunk, head): end [chunk, H, S, P] and decay [chunk, H]
//             k_ssd_carry             entry[c + 1] = decay_c entry[c] + end_c; one thread per (state element, group of
//                                     consecutive chunks): compose the group, combine the kCarryGroups groups in ascending
//                                     order through LDS, walk the group again from its true entry
//             k_ssd_out               (chunk, head): Y
//   backward  k_ssd_state<.., true>   C^T diag(e) dY: what the chunk adds to the gradient of its entry state
//             k_ssd_carry (rev)       gend[c] = the gradient arriving at the end state of chunk c
//             k_ssd_bwd               (chunk, group), the heads of the group one after the other: everything recomputed from
//                                     the operands, entry[c] and gend[c]; dB and dC are summed over the heads in ascending
//                                     order (the running sum of a position sits in the workspace between two heads)
//             k_ssd_param_reduce      dA, dD, ddt_bias: the (chunk, head) records added in ascending chunk order in fp64
// entry [chunks, H, S, P] is all that forward keeps for backward.  No atomics: every output is bitwise reproducible.
#include "common.hpp"
#include "feed_forward.hpp"
#include "piece.hpp"

namespace me {
namespace ssd {

using ffn::ff_f32x16;
using ffn::ffn_mma;
using ffn::ffn_row;
using ffn::ffn_zero;
using ffn::Frag;

constexpr int kT = 64;              // positions a chunk (me_ssd_chunk)
constexpr int kThreads = 256;       // four waves
constexpr int kWaves = kThreads / 64;
constexpr int kCarryGroups = 8;     // chunk groups of the carry kernel
constexpr int kLdsBudget = 160 * 1024;

struct Seq {                        // what every pass reads
  const void *x, *dt, *B, *C;
  int64_t x_stride, dt_stride, b_stride, c_stride;
  const float *A, *D, *bias;
  const int32_t *seg_rows, *batch_row;
  int64_t n;
  int32_t h, g, softplus, reverse;
};

struct StateArgs {                  // k_ssd_state: BWD reads C and dY in place of B and X
  Seq q;
  const void *dy;
  int64_t dy_stride;
  float *loc, *decay;               // [chunks, H, S, P], [chunks, H]
};

struct OutArgs {
  Seq q;
  const float *entry;               // [chunks, H, S, P]
  void *out;
  int64_t out_stride;
};

struct BwdArgs {
  Seq q;
  const void *dy;
  int64_t dy_stride;
  const float *entry, *gend;        // [chunks, H, S, P]
  void *dx, *ddt, *dB, *dC;         // [n, H P], [n, H], [n, G S], [n, G S] contiguous; each may be NULL
  float *bacc, *cacc;               // [chunks kT, G S]: the running head sums of dB and dC
  float *ppart;                     // [chunks, H, 3]: dA, dD, ddt_bias
};

// what a chunk knows of its positions; the first three do not depend on the head
struct Meta {
  double cum[kT];
  int32_t row[kT], seg[kT];
  float dt[kT], raw[kT], e[kT], f[kT];
  float decay;
  int32_t nt;
};

// one word of padding a row: consecutive rows start in consecutive banks
template <typename T> constexpr int ld_of(int cols) { return cols + 4 / (int)sizeof(T); }

__device__ __forceinline__ float softplus_f(float x) { return x > 20.f ? x : log1pf(expf(x)); }
__device__ __forceinline__ float sigmoid_f(float x) { return 1.f / (1.f + expf(-x)); }

// rows, starts and segment indices of the chunk (rows past nt: row 0, never read)
__device__ __forceinline__ void meta_rows(const Seq &q, int64_t chunk, Meta &m) {
  const int64_t c0 = chunk * kT;
  const int nt = (int)(q.n - c0 < kT ? q.n - c0 : kT);
  const int t = threadIdx.x;
  if (t < kT) {
    int32_t row = 0, flag = 0;
    if (t < nt) {
      const int64_t p = c0 + t;
      row = q.seg_rows[q.reverse ? q.n - 1 - p : p];
      flag = 1;
      if (p > 0) flag = q.batch_row[row] != q.batch_row[q.seg_rows[q.reverse ? q.n - p : p - 1]] ? 1 : 0;
    }
    m.row[t] = row;
    m.seg[t] = flag;
  }
  if (t == 0) m.nt = nt;
  __syncthreads();
  if (t == 0) {
    int32_t s = 0;
    for (int i = 0; i < kT; ++i) {
      s += m.seg[i];
      m.seg[i] = s;
    }
  }
  __syncthreads();
}

// dt, its running sum and the three decay vectors of head h
template <typename T>
__device__ __forceinline__ void meta_head(const Seq &q, int h, Meta &m) {
  const int t = threadIdx.x;
  if (t < kT) {
    float raw = 0.f, dt = 0.f;
    if (t < m.nt) {
      raw = (float)((const T *)q.dt)[(int64_t)m.row[t] * q.dt_stride + h];
      if (q.bias != nullptr) raw += q.bias[h];
      dt = q.softplus ? softplus_f(raw) : raw;
    }
    m.raw[t] = raw;
    m.dt[t] = dt;
  }
  __syncthreads();
  if (t == 0) {
    const double a = (double)q.A[h];
    double c = 0.0;
    for (int i = 0; i < kT; ++i) {
      c += (double)m.dt[i] * a;
      m.cum[i] = c;
    }
  }
  __syncthreads();
  if (t < kT) {
    const int last = m.seg[kT - 1];
    m.e[t] = m.seg[t] == 0 ? expf((float)m.cum[t]) : 0.f;
    m.f[t] = m.seg[t] == last ? expf((float)(m.cum[kT - 1] - m.cum[t])) : 0.f;
    if (t == 0) m.decay = last == 0 ? expf((float)m.cum[kT - 1]) : 0.f;
  }
  __syncthreads();
}

__device__ __forceinline__ float decay_ij(const Meta &m, int i, int j) {
  return (j <= i && m.seg[i] == m.seg[j]) ? expf((float)(m.cum[i] - m.cum[j])) : 0.f;
}

// dst[t][c] = scale[t] src[row_t][col0 + c] (scale NULL: 1), zero rows past nt
template <typename T>
__device__ __forceinline__ void stage_rows(T *dst, int ld, const void *src, int64_t stride, int col0, int width,
                                           const Meta &m, const float *scale) {
  for (int i = threadIdx.x; i < kT * width; i += kThreads) {
    const int t = i / width, c = i - t * width;
    float v = 0.f;
    if (t < m.nt) {
      v = (float)((const T *)src)[(int64_t)m.row[t] * stride + col0 + c];
      if (scale != nullptr) v *= scale[t];
    }
    dst[t * ld + c] = (T)v;
  }
}

// acc[m0 .. m0 + 32, n0 .. n0 + 32] += A B over K (a multiple of 16): A(m, k) = a[m ars + k aks], B(k, n) = b[k bks + n bns],
// read as UA / UB (an LDS image in the rows' type or fp32 memory) and rounded to T where T is bf16.  Lane (i, half) supplies
// k = k0 + 8 half + j of row / column i, the same k order for both operands.
template <typename T, typename UA, typename UB>
__device__ __forceinline__ void mma_seg(ff_f32x16 &acc, const UA *a, int ars, int aks, const UB *b, int bks, int bns, int K,
                                        int m0, int n0) {
  const int lane = lane_id(), i = lane & 31, k8 = 8 * (lane >> 5);
  const UA *pa = a + (int64_t)(m0 + i) * ars + (int64_t)k8 * aks;
  const UB *pb = b + (int64_t)(n0 + i) * bns + (int64_t)k8 * bks;
  for (int k0 = 0; k0 < K; k0 += 16) {
    Frag<T> fa, fb;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      fa.v[j] = (T)pa[(int64_t)(k0 + j) * aks];
      fb.v[j] = (T)pb[(int64_t)(k0 + j) * bks];
    }
    ffn_mma(acc, fa, fb);
  }
}

// The same product with every 16-wide k step in an accumulator of its own, added to acc in fp64: an fp32 accumulator over K
// terms errs by about sqrt(K) times what one over 16 does, and dA (k_ssd_bwd) sees that error of C B^T and dY X^T
template <typename T, typename UA, typename UB>
__device__ __forceinline__ void mma_seg64(double (&acc)[16], const UA *a, int ars, int aks, const UB *b, int bks, int bns,
                                          int K, int m0, int n0) {
  for (int k0 = 0; k0 < K; k0 += 16) {
    ff_f32x16 part;
    ffn_zero(part);
    mma_seg<T>(part, a + (int64_t)k0 * aks, ars, aks, b + (int64_t)k0 * bks, bks, bns, 16, m0, n0);
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[r] += (double)part[r];
  }
}

// the 32 x 32 tiles of an (mt x nt)-tile result, dealt to the waves; f(m0, n0)
template <typename F>
__device__ __forceinline__ void for_tiles(int mt, int nt, F f) {
  for (int tile = threadIdx.x >> 6; tile < mt * nt; tile += kWaves) f((tile / nt) * 32, (tile % nt) * 32);
}
// row of accumulator register r and the column of this lane
__device__ __forceinline__ int acc_row(int m0, int r) { return m0 + ffn_row(r, lane_id() >> 5); }
__device__ __forceinline__ int acc_col(int n0) { return n0 + (lane_id() & 31); }

// dst[row] = the sum of v over the tile's 32 columns, for the tile's 32 rows (butterfly over the lanes of a half).  In fp64:
// da is a difference of such sums that cancels all but the pairs on either side of a position
template <typename V>
__device__ __forceinline__ void tile_row_sums(const V (&v)[16], double *dst, int m0) {
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    double s = (double)v[r];
#pragma unroll
    for (int k = 1; k < 32; k <<= 1) s += __shfl_xor(s, k, 64);
    if ((lane_id() & 31) == 0) dst[acc_row(m0, r)] = s;
  }
}
// dst[column] = the sum of v over the tile's 32 rows
template <typename V>
__device__ __forceinline__ void tile_col_sums(const V (&v)[16], double *dst, int n0) {
  double s = 0.0;
#pragma unroll
  for (int r = 0; r < 16; ++r) s += (double)v[r];
  s += __shfl_xor(s, 32, 64);
  if (lane_id() < 32) dst[n0 + lane_id()] = s;
}

// ---- the chunk's own contribution to a state: B^T diag(f dt) X (forward), C^T diag(e) dY (backward) -------------------
template <typename T, int S, int P> constexpr int64_t state_lds() {
  return (int64_t)sizeof(Meta) + (int64_t)kT * (ld_of<T>(S) + ld_of<T>(P)) * (int64_t)sizeof(T) + 4 * kT;
}
template <typename T, int S, int P, bool BWD>
__global__ __launch_bounds__(kThreads) void k_ssd_state(StateArgs a) {
  extern __shared__ double smem[];
  constexpr int LS = ld_of<T>(S), LP = ld_of<T>(P);
  Meta &m = *reinterpret_cast<Meta *>(smem);
  T *sA = reinterpret_cast<T *>(&m + 1), *sW = sA + kT * LS;
  float *w = reinterpret_cast<float *>(sW + kT * LP);
  const Seq &q = a.q;
  const int64_t chunk = blockIdx.x;
  const int h = blockIdx.y, g = h / (q.h / q.g);
  meta_rows(q, chunk, m);
  meta_head<T>(q, h, m);
  if (threadIdx.x < kT) w[threadIdx.x] = BWD ? m.e[threadIdx.x] : m.f[threadIdx.x] * m.dt[threadIdx.x];
  __syncthreads();
  stage_rows<T>(sA, LS, BWD ? q.C : q.B, BWD ? q.c_stride : q.b_stride, g * S, S, m, nullptr);
  stage_rows<T>(sW, LP, BWD ? a.dy : q.x, BWD ? a.dy_stride : q.x_stride, h * P, P, m, w);
  __syncthreads();
  float *loc = a.loc + (chunk * q.h + h) * (int64_t)(S * P);
  for_tiles(S / 32, P / 32, [&](int m0, int n0) {
    ff_f32x16 acc;
    ffn_zero(acc);
    mma_seg<T>(acc, sA, 1, LS, sW, LP, 1, kT, m0, n0);
#pragma unroll
    for (int r = 0; r < 16; ++r) loc[acc_row(m0, r) * P + acc_col(n0)] = acc[r];
  });
  if (threadIdx.x == 0) a.decay[chunk * q.h + h] = m.decay;
}

// state[i + 1] = decay_i state[i] + loc_i over the chunks in walking order (i = c, or i = chunks - 1 - c with rev),
// state[0] = 0; out[c] = the state before chunk c is walked.  sp = S P elements a head, hsp = H S P
__global__ __launch_bounds__(64 * kCarryGroups) void k_ssd_carry(const float *__restrict__ loc,
                                                                const float *__restrict__ decay, int nchunks, int nh,
                                                                int sp, int rev, float *__restrict__ out) {
  __shared__ float sa[kCarryGroups][64], sb[kCarryGroups][64];
  const int x = threadIdx.x & 63, g = threadIdx.x >> 6;
  const int64_t hsp = (int64_t)nh * sp, el = (int64_t)blockIdx.x * 64 + x;
  const bool on = el < hsp;
  const int h = on ? (int)(el / sp) : 0;
  const int L = (nchunks + kCarryGroups - 1) / kCarryGroups;
  const int i0 = g * L < nchunks ? g * L : nchunks, i1 = i0 + L < nchunks ? i0 + L : nchunks;
  float av = 1.f, b = 0.f;
  if (on) {
    for (int i = i0; i < i1; ++i) {
      const int64_t c = rev ? nchunks - 1 - i : i;
      const float d = decay[c * nh + h];
      b = d * b + loc[c * hsp + el];
      av *= d;
    }
  }
  sa[g][x] = av;
  sb[g][x] = b;
  __syncthreads();
  if (!on) return;
  float e = 0.f;
  for (int gg = 0; gg < g; ++gg) e = sa[gg][x] * e + sb[gg][x];
  for (int i = i0; i < i1; ++i) {
    const int64_t c = rev ? nchunks - 1 - i : i;
    out[c * hsp + el] = e;
    e = decay[c * nh + h] * e + loc[c * hsp + el];
  }
}

// ---- Y of a chunk and head ------------------------------------------------------------------------------------------------
template <typename T, int S, int P> constexpr int64_t out_lds() {
  return (int64_t)sizeof(Meta) + (int64_t)kT * (2 * ld_of<T>(S) + ld_of<T>(P) + ld_of<T>(kT)) * (int64_t)sizeof(T);
}
template <typename T, int S, int P>
__global__ __launch_bounds__(kThreads) void k_ssd_out(OutArgs a) {
  extern __shared__ double smem[];
  constexpr int LS = ld_of<T>(S), LP = ld_of<T>(P), LT = ld_of<T>(kT);
  Meta &m = *reinterpret_cast<Meta *>(smem);
  T *sB = reinterpret_cast<T *>(&m + 1), *sC = sB + kT * LS, *sX = sC + kT * LS, *sM = sX + kT * LP;
  const Seq &q = a.q;
  const int64_t chunk = blockIdx.x;
  const int h = blockIdx.y, g = h / (q.h / q.g);
  meta_rows(q, chunk, m);
  meta_head<T>(q, h, m);
  stage_rows<T>(sB, LS, q.B, q.b_stride, g * S, S, m, nullptr);
  stage_rows<T>(sC, LS, q.C, q.c_stride, g * S, S, m, nullptr);
  stage_rows<T>(sX, LP, q.x, q.x_stride, h * P, P, m, nullptr);
  __syncthreads();
  for_tiles(kT / 32, kT / 32, [&](int m0, int n0) {       // M = (C B^T) o L diag(dt)
    ff_f32x16 acc;
    ffn_zero(acc);
    mma_seg<T>(acc, sC, LS, 1, sB, 1, LS, S, m0, n0);
    const int j = acc_col(n0);
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int i = acc_row(m0, r);
      sM[i * LT + j] = (T)(acc[r] * decay_ij(m, i, j) * m.dt[j]);
    }
  });
  __syncthreads();
  const float *entry = a.entry + (chunk * q.h + h) * (int64_t)(S * P);
  const float dsk = q.D != nullptr ? q.D[h] : 0.f;
  for_tiles(kT / 32, P / 32, [&](int m0, int n0) {        // Y = M X + diag(e) C entry + D X
    ff_f32x16 acc, acc2;
    ffn_zero(acc);
    ffn_zero(acc2);
    mma_seg<T>(acc, sM, LT, 1, sX, LP, 1, kT, m0, n0);
    mma_seg<T>(acc2, sC, LS, 1, entry, P, 1, S, m0, n0);
    const int p = acc_col(n0);
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int i = acc_row(m0, r);
      if (i < m.nt)
        ((T *)a.out)[(int64_t)m.row[i] * a.out_stride + h * P + p] =
            (T)(acc[r] + m.e[i] * acc2[r] + dsk * (float)sX[i * LP + p]);
    }
  });
}

// ---- every gradient of a chunk and group but the merge of the parameter gradients over the chunks -------------------------
// With R = dY X^T, Mf = (C B^T) o L, dG = R diag(dt) o L, and E = entry[c], Gn = gend[c]:
//   dC = dG B + diag(e) dY E^T                    dB = dG^T C + diag(f dt) X Gn^T
//   dU = Mf^T dY + diag(f) B Gn                   dx = dt dU + D dY
//   q_i = d/dcum_i = rowsum_i(N) - colsum_i(N) + e_i dY_i . (C E)_i - f_i dt_i x_i . (B Gn)_i,   N = R diag(dt) o Mf
//   q_last += sum_j f_j dt_j x_j . (B Gn)_j + decay (Gn . E)
//   da_t = sum_{i >= t} q_i;   ddt_t = da_t A + dU_t . x_t;   dA = sum_t da_t dt_t;   dD = sum dY o X
template <typename T, int S, int P> constexpr int64_t bwd_lds() {
  return (int64_t)sizeof(Meta) +
         (int64_t)kT * (2 * ld_of<T>(S) + 2 * ld_of<T>(P) + 2 * ld_of<T>(kT)) * (int64_t)sizeof(T) +
         10 * kT * (int64_t)sizeof(double) + (int64_t)(kT + kThreads) * (int64_t)sizeof(float);
}
template <typename T, int S, int P>
__global__ __launch_bounds__(kThreads) void k_ssd_bwd(BwdArgs a) {
  extern __shared__ double smem[];
  constexpr int LS = ld_of<T>(S), LP = ld_of<T>(P), LT = ld_of<T>(kT);
  Meta &m = *reinterpret_cast<Meta *>(smem);
  double *rowN = reinterpret_cast<double *>(&m + 1);        // [2][kT] each: one record a column (row) tile
  double *colN = rowN + 2 * kT, *r1 = colN + 2 * kT, *r2 = r1 + 2 * kT, *dd = r2 + 2 * kT;
  T *sB = reinterpret_cast<T *>(dd + 2 * kT), *sC = sB + kT * LS, *sX = sC + kT * LS, *sdY = sX + kT * LP;
  T *sMf = sdY + kT * LP, *sdG = sMf + kT * LT;
  float *dDrow = reinterpret_cast<float *>(sdG + kT * LT), *red = dDrow + kT;   // [kT], [kThreads]
  const Seq &q = a.q;
  const int64_t chunk = blockIdx.x;
  const int g = blockIdx.y, hpg = q.h / q.g, tid = threadIdx.x;
  meta_rows(q, chunk, m);
  stage_rows<T>(sB, LS, q.B, q.b_stride, g * S, S, m, nullptr);
  stage_rows<T>(sC, LS, q.C, q.c_stride, g * S, S, m, nullptr);
  for (int i = tid; i < 10 * kT; i += kThreads) rowN[i] = 0.0;   // P = 32 leaves the second records unwritten
  for (int hh = 0; hh < hpg; ++hh) {
    const int h = g * hpg + hh;
    __syncthreads();                                       // the head before has been read out of LDS
    meta_head<T>(q, h, m);
    stage_rows<T>(sX, LP, q.x, q.x_stride, h * P, P, m, nullptr);
    stage_rows<T>(sdY, LP, a.dy, a.dy_stride, h * P, P, m, nullptr);
    __syncthreads();
    const float *E = a.entry + (chunk * q.h + h) * (int64_t)(S * P);
    const float *Gn = a.gend + (chunk * q.h + h) * (int64_t)(S * P);
    const float dsk = q.D != nullptr ? q.D[h] : 0.f;
    if (tid < kT) {                                        // dD of the row; then Gn . E of the thread's elements
      float s = 0.f;
      for (int p = 0; p < P; ++p) s += (float)sdY[tid * LP + p] * (float)sX[tid * LP + p];
      dDrow[tid] = s;
    }
    {
      float s = 0.f;
      for (int i = tid; i < S * P; i += kThreads) s += Gn[i] * E[i];
      red[tid] = s;
    }
    for_tiles(kT / 32, kT / 32, [&](int m0, int n0) {      // Mf, dG and the sums of N
      double acc[16], acc2[16], nv[16];                   // N in fp64: its sums cancel (see tile_row_sums)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[r] = acc2[r] = 0.0;
      if constexpr (sizeof(T) == 4) {                     // fp32 rows: short fp32 sums (see mma_seg64)
        mma_seg64<T>(acc, sC, LS, 1, sB, 1, LS, S, m0, n0);
        mma_seg64<T>(acc2, sdY, LP, 1, sX, 1, LP, P, m0, n0);
      } else {
        ff_f32x16 a32, b32;
        ffn_zero(a32);
        ffn_zero(b32);
        mma_seg<T>(a32, sC, LS, 1, sB, 1, LS, S, m0, n0);
        mma_seg<T>(b32, sdY, LP, 1, sX, 1, LP, P, m0, n0);
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[r] = (double)a32[r], acc2[r] = (double)b32[r];
      }
      const int j = acc_col(n0);
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int i = acc_row(m0, r);
        const float l = decay_ij(m, i, j);
        const double mf = acc[r] * (double)l, rd = acc2[r] * (double)m.dt[j];
        sMf[i * LT + j] = (T)(float)mf;
        sdG[i * LT + j] = (T)(float)(rd * (double)l);
        nv[r] = rd * mf;
      }
      tile_row_sums(nv, rowN + (n0 / 32) * kT, m0);
      tile_col_sums(nv, colN + (m0 / 32) * kT, n0);
    });
    __syncthreads();
    // the running head sum of a position's dB / dC: written and read again by the same lane
    auto merge = [&](float v, int i, int s, float *accum, void *dst) {
      const int64_t o = (chunk * kT + i) * (int64_t)(q.g * S) + g * S + s;
      if (hh > 0) v += accum[o];
      if (hh + 1 < hpg) accum[o] = v;
      else if (i < m.nt) ((T *)dst)[(int64_t)m.row[i] * (q.g * S) + g * S + s] = (T)v;
    };
    if (a.dC != nullptr)
      for_tiles(kT / 32, S / 32, [&](int m0, int n0) {
        ff_f32x16 acc, acc2;
        ffn_zero(acc);
        ffn_zero(acc2);
        mma_seg<T>(acc, sdG, LT, 1, sB, LS, 1, kT, m0, n0);
        mma_seg<T>(acc2, sdY, LP, 1, E, 1, P, P, m0, n0);
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const int i = acc_row(m0, r);
          merge(acc[r] + m.e[i] * acc2[r], i, acc_col(n0), a.cacc, a.dC);
        }
      });
    if (a.dB != nullptr)
      for_tiles(kT / 32, S / 32, [&](int m0, int n0) {
        ff_f32x16 acc, acc2;
        ffn_zero(acc);
        ffn_zero(acc2);
        mma_seg<T>(acc, sdG, 1, LT, sC, LS, 1, kT, m0, n0);
        mma_seg<T>(acc2, sX, LP, 1, Gn, 1, P, P, m0, n0);
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const int i = acc_row(m0, r);
          merge(acc[r] + m.f[i] * m.dt[i] * acc2[r], i, acc_col(n0), a.bacc, a.dB);
        }
      });
    for_tiles(kT / 32, P / 32, [&](int m0, int n0) {       // dU, dx and the row sums that da and ddt need
      ff_f32x16 acc, acc2, acc3;
      ffn_zero(acc);
      ffn_zero(acc2);
      ffn_zero(acc3);
      mma_seg<T>(acc, sMf, 1, LT, sdY, LP, 1, kT, m0, n0);
      mma_seg<T>(acc2, sB, LS, 1, Gn, P, 1, S, m0, n0);
      mma_seg<T>(acc3, sC, LS, 1, E, P, 1, S, m0, n0);
      const int p = acc_col(n0);
      float v1[16], v2[16], vd[16];
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int i = acc_row(m0, r);
        const float x = (float)sX[i * LP + p], dy = (float)sdY[i * LP + p];
        const float du = acc[r] + m.f[i] * acc2[r];
        v1[r] = m.e[i] * acc3[r] * dy;
        v2[r] = m.f[i] * m.dt[i] * acc2[r] * x;
        vd[r] = du * x;
        if (a.dx != nullptr && i < m.nt)
          ((T *)a.dx)[(int64_t)m.row[i] * (q.h * P) + h * P + p] = (T)(m.dt[i] * du + dsk * dy);
      }
      tile_row_sums(v1, r1 + (n0 / 32) * kT, m0);
      tile_row_sums(v2, r2 + (n0 / 32) * kT, m0);
      tile_row_sums(vd, dd + (n0 / 32) * kT, m0);
    });
    __syncthreads();
    if (tid == 0) {                                        // one lane, one order: the chunk's suffix sums in fp64
      double ge = 0.0, tail = 0.0, dD = 0.0, dA = 0.0, dbias = 0.0;
      for (int i = 0; i < kThreads; ++i) ge += (double)red[i];
      for (int t = 0; t < kT; ++t) {
        tail += r2[t] + r2[kT + t];
        dD += (double)dDrow[t];
      }
      double suffix = tail + (double)m.decay * ge;
      const double av = (double)q.A[h];
      for (int t = kT - 1; t >= 0; --t) {
        suffix += (rowN[t] + rowN[kT + t]) - (colN[t] + colN[kT + t]) + (r1[t] + r1[kT + t]) - (r2[t] + r2[kT + t]);
        if (t < m.nt) {
          float ddt = (float)(suffix * av + (dd[t] + dd[kT + t]));
          if (q.softplus && m.raw[t] <= 20.f) ddt *= sigmoid_f(m.raw[t]);
          if (a.ddt != nullptr) ((T *)a.ddt)[(int64_t)m.row[t] * q.h + h] = (T)ddt;
          dbias += (double)ddt;
          dA += suffix * (double)m.dt[t];
        }
      }
      float *pp = a.ppart + (chunk * q.h + h) * 3;
      pp[0] = (float)dA;
      pp[1] = (float)dD;
      pp[2] = (float)dbias;
    }
  }
}

// dA, dD, ddt_bias [H] = the chunks' records, added in ascending chunk order in fp64
__global__ __launch_bounds__(256) void k_ssd_param_reduce(const float *__restrict__ part, int nchunks, int nh,
                                                          float *__restrict__ dA, float *__restrict__ dD,
                                                          float *__restrict__ dbias) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= nh * 3) return;
  double r = 0.0;
  for (int64_t c = 0; c < nchunks; ++c) r += (double)part[c * nh * 3 + i];
  float *dst = i % 3 == 0 ? dA : i % 3 == 1 ? dD : dbias;
  if (dst != nullptr) dst[i / 3] = (float)r;
}

// ---- launch policy (host) -------------------------------------------------------------------------------------------------
inline int64_t chunks_of(int64_t n) { return ceil_div(n, kT); }

struct Workspace {                  // offsets in floats
  int64_t loc, decay, gend, bacc, cacc, ppart, total;
};
inline Workspace workspace_of(int64_t n, int h, int p, int s, int g, bool backward) {
  Workspace w{};
  const int64_t nch = chunks_of(n);
  int64_t o = 0;
  w.loc = o, o += nch * h * s * p;
  w.decay = o, o += nch * h;
  if (backward) {
    w.gend = o, o += nch * h * s * p;
    w.bacc = o, o += nch * kT * g * s;
    w.cacc = o, o += nch * kT * g * s;
    w.ppart = o, o += nch * h * 3;
  }
  w.total = o;
  return w;
}

template <typename K, typename A>
int launch(K fn, int64_t lds, dim3 grid, const A &a, hipStream_t stream) {
  ME_CHECK(lds <= kLdsBudget, "the chunk images do not fit into LDS");
  if (ffn::allow_lds(fn, lds) != 0) return 1;
  hipLaunchKernelGGL(fn, grid, dim3(kThreads), (size_t)lds, stream, a);
  ME_LAUNCH_CHECK();
  return 0;
}

inline int carry(const float *loc, const float *decay, int64_t nch, const Seq &q, int s, int p, int rev, float *out,
                 hipStream_t stream) {
  hipLaunchKernelGGL(k_ssd_carry, dim3((unsigned)ceil_div((int64_t)q.h * s * p, 64)), dim3(64 * kCarryGroups), 0, stream,
                     loc, decay, (int)nch, q.h, s * p, rev, out);
  ME_LAUNCH_CHECK();
  return 0;
}

template <typename T, int S, int P>
int forward(const Seq &q, float *entry, void *out, int64_t out_stride, float *ws, hipStream_t stream) {
  const int64_t nch = chunks_of(q.n);
  const Workspace w = workspace_of(q.n, q.h, P, S, q.g, false);
  const dim3 grid((unsigned)nch, (unsigned)q.h);
  const StateArgs sa{q, nullptr, 0, ws + w.loc, ws + w.decay};
  if (launch(k_ssd_state<T, S, P, false>, state_lds<T, S, P>(), grid, sa, stream) != 0) return 1;
  if (carry(ws + w.loc, ws + w.decay, nch, q, S, P, 0, entry, stream) != 0) return 1;
  const OutArgs oa{q, entry, out, out_stride};
  return launch(k_ssd_out<T, S, P>, out_lds<T, S, P>(), grid, oa, stream);
}

template <typename T, int S, int P>
int backward(BwdArgs a, float *dA, float *dD, float *dbias, float *ws, hipStream_t stream) {
  const Seq &q = a.q;
  const int64_t nch = chunks_of(q.n);
  const Workspace w = workspace_of(q.n, q.h, P, S, q.g, true);
  const StateArgs sa{q, a.dy, a.dy_stride, ws + w.loc, ws + w.decay};
  if (launch(k_ssd_state<T, S, P, true>, state_lds<T, S, P>(), dim3((unsigned)nch, (unsigned)q.h), sa, stream) != 0)
    return 1;
  if (carry(ws + w.loc, ws + w.decay, nch, q, S, P, 1, ws + w.gend, stream) != 0) return 1;
  a.gend = ws + w.gend;
  a.bacc = ws + w.bacc;
  a.cacc = ws + w.cacc;
  a.ppart = ws + w.ppart;
  if (launch(k_ssd_bwd<T, S, P>, bwd_lds<T, S, P>(), dim3((unsigned)nch, (unsigned)q.g), a, stream) != 0) return 1;
  if (dA != nullptr || dD != nullptr || dbias != nullptr) {
    hipLaunchKernelGGL(k_ssd_param_reduce, dim3((unsigned)ceil_div(q.h * 3, 256)), dim3(256), 0, stream, a.ppart, (int)nch,
                       q.h, dA, dD, dbias);
    ME_LAUNCH_CHECK();
  }
  return 0;
}

// T, S (64 | 128) and P (32 | 64) of a call
#define ME_SSD_DISPATCH(is_bf16, s, p, FN, ...)                                                          \
  do {                                                                                                   \
    if (is_bf16) {                                                                                       \
      if (s == 64) return p == 32 ? FN<__bf16, 64, 32>(__VA_ARGS__) : FN<__bf16, 64, 64>(__VA_ARGS__);   \
      return p == 32 ? FN<__bf16, 128, 32>(__VA_ARGS__) : FN<__bf16, 128, 64>(__VA_ARGS__);              \
    }                                                                                                    \
    if (s == 64) return p == 32 ? FN<float, 64, 32>(__VA_ARGS__) : FN<float, 64, 64>(__VA_ARGS__);       \
    return p == 32 ? FN<float, 128, 32>(__VA_ARGS__) : FN<float, 128, 64>(__VA_ARGS__);                  \
  } while (0)

}  // namespace ssd
}  // namespace me

using namespace me;

// the checks both directions share; rows of n > 0 follow in the callers
#define ME_SSD_CHECK_SHAPE(n, h, p, s, g)                                                                        \
  ME_CHECK(n >= 0 && n < ((int64_t)1 << 31), "n must be in [0, 2^31)");                                          \
  ME_CHECK(me_ssd_supported(h, p, s, g, 0) != 0,                                                                 \
           "the kernels serve h >= 1 heads of width 32 or 64, 64 or 128 states and g groups dividing h");        \
  ME_CHECK(x_stride >= (int64_t)h * p && dt_stride >= h && b_stride >= (int64_t)g * s && c_stride >= (int64_t)g * s, \
           "a row stride must be at least the row width")

extern "C" {

int32_t me_ssd_supported(int32_t h, int32_t p, int32_t s, int32_t g, int32_t is_bf16) {
  (void)is_bf16;
  return (h >= 1 && g >= 1 && h % g == 0 && (p == 32 || p == 64) && (s == 64 || s == 128)) ? 1 : 0;
}

int32_t me_ssd_chunk(void) { return ssd::kT; }

int64_t me_ssd_workspace_bytes(int64_t n, int32_t h, int32_t p, int32_t s, int32_t g, int32_t backward) {
  if (n <= 0 || h < 1 || p < 1 || s < 1 || g < 1) return 0;
  return ssd::workspace_of(n, h, p, s, g, backward != 0).total * (int64_t)sizeof(float);
}

int me_ssd_forward(const void *x_dev, const void *dt_dev, const void *b_dev, const void *c_dev, int32_t is_bf16,
                   int64_t x_stride, int64_t dt_stride, int64_t b_stride, int64_t c_stride, const float *a_dev,
                   const float *d_dev, const float *dt_bias_dev, int32_t dt_softplus, const int32_t *seg_rows_dev,
                   const int32_t *batch_row_dev, int32_t reverse, int64_t n, int32_t h, int32_t p, int32_t s, int32_t g,
                   void *out_dev, int64_t out_stride, float *entry_dev, void *workspace_dev, int64_t workspace_bytes,
                   void *stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  ME_SSD_CHECK_SHAPE(n, h, p, s, g);
  ME_CHECK(out_stride >= (int64_t)h * p, "a row stride must be at least the row width");
  if (n == 0) return 0;
  ME_CHECK(x_dev != nullptr && dt_dev != nullptr && b_dev != nullptr && c_dev != nullptr && a_dev != nullptr &&
               out_dev != nullptr && entry_dev != nullptr,
           "x, dt, B, C, A, out and entry must be given");
  ME_CHECK(seg_rows_dev != nullptr && batch_row_dev != nullptr, "the sequence rows and the instance of every row must be given");
  ME_CHECK(workspace_dev != nullptr && workspace_bytes >= me_ssd_workspace_bytes(n, h, p, s, g, 0),
           "the workspace is smaller than me_ssd_workspace_bytes");
  const int elem = is_bf16 ? 2 : 4;
  ME_CHECK(aligned({x_dev, dt_dev, b_dev, c_dev, out_dev}, elem) &&
               aligned({a_dev, d_dev, dt_bias_dev, seg_rows_dev, batch_row_dev, entry_dev, workspace_dev}, 4),
           "the operands must be aligned to their element");
  const ssd::Seq q{x_dev, dt_dev, b_dev, c_dev, x_stride, dt_stride, b_stride, c_stride, a_dev, d_dev, dt_bias_dev,
                   seg_rows_dev, batch_row_dev, n, h, g, dt_softplus ? 1 : 0, reverse ? 1 : 0};
  ME_SSD_DISPATCH(is_bf16, s, p, ssd::forward, q, entry_dev, out_dev, out_stride, (float *)workspace_dev, stream);
}

int me_ssd_backward(const void *x_dev, const void *dt_dev, const void *b_dev, const void *c_dev, const void *dout_dev,
                    int32_t is_bf16, int64_t x_stride, int64_t dt_stride, int64_t b_stride, int64_t c_stride,
                    int64_t dout_stride, const float *a_dev, const float *d_dev, const float *dt_bias_dev,
                    int32_t dt_softplus, const int32_t *seg_rows_dev, const int32_t *batch_row_dev, int32_t reverse,
                    int64_t n, int32_t h, int32_t p, int32_t s, int32_t g, const float *entry_dev, void *dx_dev,
                    void *ddt_dev, void *db_dev, void *dc_dev, float *da_dev, float *dd_dev, float *ddt_bias_dev,
                    void *workspace_dev, int64_t workspace_bytes, void *stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  ME_SSD_CHECK_SHAPE(n, h, p, s, g);
  ME_CHECK(dout_stride >= (int64_t)h * p, "a row stride must be at least the row width");
  ME_CHECK(dd_dev == nullptr || d_dev != nullptr, "the gradient of D needs D");
  ME_CHECK(ddt_bias_dev == nullptr || dt_bias_dev != nullptr, "the gradient of dt_bias needs dt_bias");
  if (n == 0) {                                       // no rows: the parameter gradients are sums of no records
    if (da_dev != nullptr || dd_dev != nullptr || ddt_bias_dev != nullptr) {
      hipLaunchKernelGGL(ssd::k_ssd_param_reduce, dim3((unsigned)ceil_div(h * 3, 256)), dim3(256), 0, stream,
                         (const float *)nullptr, 0, h, da_dev, dd_dev, ddt_bias_dev);
      ME_LAUNCH_CHECK();
    }
    return 0;
  }
  ME_CHECK(x_dev != nullptr && dt_dev != nullptr && b_dev != nullptr && c_dev != nullptr && a_dev != nullptr &&
               dout_dev != nullptr && entry_dev != nullptr,
           "x, dt, B, C, A, dout and entry must be given");
  ME_CHECK(seg_rows_dev != nullptr && batch_row_dev != nullptr, "the sequence rows and the instance of every row must be given");
  ME_CHECK(workspace_dev != nullptr && workspace_bytes >= me_ssd_workspace_bytes(n, h, p, s, g, 1),
           "the workspace is smaller than me_ssd_workspace_bytes");
  const int elem = is_bf16 ? 2 : 4;
  ME_CHECK(aligned({x_dev, dt_dev, b_dev, c_dev, dout_dev, dx_dev, ddt_dev, db_dev, dc_dev}, elem) &&
               aligned({a_dev, d_dev, dt_bias_dev, seg_rows_dev, batch_row_dev, entry_dev, da_dev, dd_dev, ddt_bias_dev,
                        workspace_dev}, 4),
           "the operands must be aligned to their element");
  const ssd::BwdArgs a{{x_dev, dt_dev, b_dev, c_dev, x_stride, dt_stride, b_stride, c_stride, a_dev, d_dev, dt_bias_dev,
                        seg_rows_dev, batch_row_dev, n, h, g, dt_softplus ? 1 : 0, reverse ? 1 : 0},
                       dout_dev, dout_stride, entry_dev, nullptr, dx_dev, ddt_dev, db_dev, dc_dev, nullptr, nullptr, nullptr};
  ME_SSD_DISPATCH(is_bf16, s, p, ssd::backward, a, da_dev, dd_dev, ddt_bias_dev, (float *)workspace_dev, stream);
}

}  // extern "C"
