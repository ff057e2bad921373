// Fused two-layer MLP over the rows of a feature matrix for gfx950 (MI355X): y = act(x W1^T + b1) W2^T + b2 with
// x [n, C], W1 [Hd, C], W2 [Cout, Hd] (torch.nn.Linear's layouts).  The hidden matrix [n, Hd] never reaches memory, in
// either direction: every kernel recomputes the 32-wide chunk of it that it needs from x.
//
//   k_ffn_fwd     row-stationary.  A workgroup of four waves owns 128 rows, a wave 32 of them; the wave's rows of x stay
//                 in registers as B fragments, the accumulators of y stay in registers over the whole walk over Hd.
//   k_ffn_bwd_x   the same body with one more first product: Z^T is recomputed, dH^T = W2^T[chunk, :] dY^T, dZ = dH act'(Z),
//                 dX^T += W1^T[:, chunk] dZ^T.  The transposed weights come from k_ffn_transpose (one launch per backward).
//   k_ffn_bwd_w   hidden-stationary.  A workgroup owns (32-wide hidden chunk, row split) and walks its rows 128 at a time,
//                 a wave 32 of them; dW1[chunk, :], dW2[:, chunk] and db1[chunk] of the wave's rows stay in registers and
//                 are written once as an fp32 partial image per (split, wave).  db2 rides in the chunk-0 workgroups.
//   k_ffn_reduce  sums the partial images in ascending (split, wave) order and rounds once to the parameter type.
//
// One 32x32 MFMA shape serves both dtypes, as in attention.hip: v_mfma_f32_32x32x16_bf16 on bf16 rows, the exact
// v_mfma_f32_32x32x2_f32 on fp32 rows; C/D lane map: column = lane & 31, row = (reg & 3) + 8 (reg >> 2) + 4 (lane >> 5).
// The row-stationary kernels take every product transposed, so that a row of x is the COLUMN (lane & 31) of every tile:
//   Z^T[32 hidden x 32 rows] = W1[chunk, :] X^T     A = W1's row-major rows from LDS, B = the wave's x fragments
// and the 16 accumulator registers, after bias and activation in fp32, are the two k-steps of the B operand of
//   Y^T[32 t .., rows] += W2[32 t .., chunk] H^T    A read from LDS in the permuted k order (ffn_load44)
// with no lane movement and no LDS: registers 8 s .. 8 s + 7 are k-step s, element j of lane half h being hidden unit
// 16 s + 8 (j >> 2) + 4 h + (j & 3).  The weight-gradient kernel sums over ROWS, so there the first products are taken
// plain (Z[32 rows x 32 hidden] = X W1[chunk, :]^T, the hidden unit on the lane) and the same identity feeds
//   dW1^T[32 t .., chunk] += X^T[32 t .., rows] dZ,   dW2[32 t .., chunk] += dY^T[32 t .., rows] H
// whose A operands are read from a wave-private transposed LDS image of the wave's 32 rows.
// The hidden activation (H, dZ) is rounded once to bf16 where it becomes an MFMA operand on bf16 rows and stays fp32 on fp32
// rows; all accumulation is fp32; outputs are rounded once.  No atomics, fixed summation orders: bitwise reproducible.
// The weight blocks of a chunk are staged into LDS in 16-byte pieces once per workgroup, double-buffered in the
// row-stationary kernels (one barrier per chunk).  A partial last row block clamps the row index and masks the store (the
// weight-gradient kernel zeroes the clamped rows of x and dy instead).
// Widths: C and Cout multiples of 32 up to ME_FFN_MAX_WIDTH_BF16 / ME_FFN_MAX_WIDTH_F32, Hd any multiple of 32.  A kernel is
// instantiated per (dtype, MT) with MT = 2 | 4 | 8 the register tiles that hold max(C, Cout) / 32; tiles beyond the actual
// widths are skipped by wave-uniform branches.
#include "feed_forward.hpp"

namespace me {
namespace ffn {

constexpr int kBiasBytes = 2 * 32 * (int)sizeof(float);

// GRAD: hv = dh * act'(z + bias) and hact = act(z + bias); else hv = act(z + bias).  bias[i]: of register i.
template <int A, bool GRAD>
__device__ __forceinline__ void hidden_one(const ff_f32x16 &z, const ff_f32x16 &dh, const float (&bias)[16],
                                           float (&hv)[16], float (&hact)[16]) {
#pragma unroll
  for (int i = 0; i < 16; ++i) {
    const float v = z[i] + bias[i];
    if constexpr (GRAD) {
      hv[i] = dh[i] * act_g<A>(v);
      hact[i] = act_f<A>(v);
    } else {
      hv[i] = act_f<A>(v);
    }
  }
}
template <bool GRAD>
__device__ __forceinline__ void hidden(int act, const ff_f32x16 &z, const ff_f32x16 &dh, const float (&bias)[16],
                                       float (&hv)[16], float (&hact)[16]) {
  switch (act) {   // wave-uniform
    case ME_FFN_RELU: hidden_one<ME_FFN_RELU, GRAD>(z, dh, bias, hv, hact); break;
    case ME_FFN_GELU: hidden_one<ME_FFN_GELU, GRAD>(z, dh, bias, hv, hact); break;
    case ME_FFN_GELU_TANH: hidden_one<ME_FFN_GELU_TANH, GRAD>(z, dh, bias, hv, hact); break;
    default: hidden_one<ME_FFN_SILU, GRAD>(z, dh, bias, hv, hact); break;
  }
}

// ---- row-stationary: forward and input gradient ----------------------------------------------------------------------
// forward:  x, wa = W1 [hd, c], wc = W2 [cout, hd], b1, b2 -> out = y [n, cout]
// backward: x, g = dy [n, cout], wa = W1, wb = W2^T [hd, cout], wc = W1^T [c, hd], b1 -> out = dx [n, c]
template <typename T> struct RowsArgs {
  const T *x, *g, *wa, *wb, *wc, *b1, *b2;
  T *out;
  int64_t n;
  int c, hd, cout, act;
};

// LDS: the two bias chunks, then two buffers of [32][c + PAD] (wa), [32][cout + PAD] (wb, backward), [co][32 + PAD] (wc)
static inline int64_t rows_lds_bytes(int elem, int c, int cout, bool bwd) {
  const int pad = 16 / elem, co = bwd ? c : cout;
  const int64_t buf = 32 * (c + pad) + (bwd ? 32 * (cout + pad) : 0) + (int64_t)co * (32 + pad);
  return kBiasBytes + 2 * buf * elem;
}

template <typename T, int MT, bool BWD> __device__ __forceinline__ void ffn_rows(const RowsArgs<T> &a) {
  constexpr int PAD = FfnT<T>::PAD;
  extern __shared__ __attribute__((aligned(16))) unsigned char s_ffn[];
  float *s_bias = reinterpret_cast<float *>(s_ffn);   // [2][32]
  T *s_buf = reinterpret_cast<T *>(s_ffn + kBiasBytes);
  const int c = a.c, hd = a.hd, cout = a.cout, co = BWD ? c : cout;
  const int lda = c + PAD, ldb = cout + PAD, ldc = 32 + PAD;
  const int buf_elems = 32 * lda + (BWD ? 32 * ldb : 0) + co * ldc;
  const int nka = c / 16, nkb = cout / 16, nto = co / 32, nchunks = hd / 32;
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, r = lane & 31, h = lane >> 5;
  const int64_t row = (int64_t)blockIdx.x * kRows + wave * 32 + r, rc = row < a.n ? row : a.n - 1;

  Frag<T> xf[2 * MT], gf[BWD ? 2 * MT : 1];
#pragma unroll
  for (int k = 0; k < 2 * MT; ++k)
    if (k < nka) xf[k] = ffn_load8(a.x + rc * c + 16 * k + 8 * h);
  if constexpr (BWD) {
#pragma unroll
    for (int k = 0; k < 2 * MT; ++k)
      if (k < nkb) gf[k] = ffn_load8(a.g + rc * cout + 16 * k + 8 * h);
  }
  ff_f32x16 o[MT];
#pragma unroll
  for (int t = 0; t < MT; ++t) ffn_zero(o[t]);

  auto stage_chunk = [&](int j) {
    T *sa = s_buf + (j & 1) * buf_elems, *sb = sa + 32 * lda, *sc = sb + (BWD ? 32 * ldb : 0);
    stage<T>(a.wa + (int64_t)32 * j * c, c, 32, c, sa, lda);
    if constexpr (BWD) stage<T>(a.wb + (int64_t)32 * j * cout, cout, 32, cout, sb, ldb);
    stage<T>(a.wc + 32 * j, hd, co, 32, sc, ldc);
    if (threadIdx.x < 32) s_bias[(j & 1) * 32 + threadIdx.x] = a.b1 != nullptr ? (float)a.b1[32 * j + threadIdx.x] : 0.f;
  };
  stage_chunk(0);
  for (int j = 0; j < nchunks; ++j) {
    __syncthreads();   // chunk j is staged, and every wave is done with chunk j - 1, whose buffer chunk j + 1 takes
    if (j + 1 < nchunks) stage_chunk(j + 1);
    const T *sa = s_buf + (j & 1) * buf_elems, *sb = sa + 32 * lda, *sc = sb + (BWD ? 32 * ldb : 0);
    ff_f32x16 z;
    ffn_zero(z);
#pragma unroll
    for (int k = 0; k < 2 * MT; ++k)
      if (k < nka) ffn_mma(z, ffn_load8(sa + r * lda + 16 * k + 8 * h), xf[k]);   // Z^T[hidden][row]
    float bias[16], hv[16], unused[16];
#pragma unroll
    for (int i = 0; i < 16; ++i) bias[i] = s_bias[(j & 1) * 32 + ffn_row(i, h)];
    if constexpr (BWD) {
      ff_f32x16 dh;
      ffn_zero(dh);
#pragma unroll
      for (int k = 0; k < 2 * MT; ++k)
        if (k < nkb) ffn_mma(dh, ffn_load8(sb + r * ldb + 16 * k + 8 * h), gf[k]);   // dH^T[hidden][row]
      hidden<true>(a.act, z, dh, bias, hv, unused);
    } else {
      hidden<false>(a.act, z, z, bias, hv, unused);
    }
#pragma unroll
    for (int s = 0; s < 2; ++s) {
      const Frag<T> hf = ffn_acc_frag<T>(hv, s);
#pragma unroll
      for (int t = 0; t < MT; ++t)   // out^T[channel][row] += wc[channel][hidden] hidden^T[hidden][row]
        if (t < nto) ffn_mma(o[t], ffn_load44(sc + (t * 32 + r) * ldc + 16 * s + 4 * h), hf);
    }
  }
  if (row >= a.n) return;
  T *base = a.out + row * co;
#pragma unroll
  for (int t = 0; t < MT; ++t) {
    if (t >= nto) continue;
#pragma unroll
    for (int g = 0; g < 4; ++g) {
      const int ch = t * 32 + 8 * g + 4 * h;
      float b[4] = {0.f, 0.f, 0.f, 0.f};
      if (!BWD && a.b2 != nullptr) {
#pragma unroll
        for (int e = 0; e < 4; ++e) b[e] = (float)a.b2[ch + e];
      }
      ffn_store4(base + ch, o[t][4 * g] + b[0], o[t][4 * g + 1] + b[1], o[t][4 * g + 2] + b[2], o[t][4 * g + 3] + b[3]);
    }
  }
}

template <typename T, int MT> __global__ __launch_bounds__(kThreads) void k_ffn_fwd(const RowsArgs<T> a) {
  ffn_rows<T, MT, false>(a);
}
template <typename T, int MT> __global__ __launch_bounds__(kThreads) void k_ffn_bwd_x(const RowsArgs<T> a) {
  ffn_rows<T, MT, true>(a);
}

// ---- weight gradient: hidden-stationary -------------------------------------------------------------------------------
// floats of one partial image: [dW1 hd x c | dW2 cout x hd | db1 hd | db2 cout]
static __host__ __device__ __forceinline__ int64_t image_floats(int c, int hd, int cout) {
  return (int64_t)hd * c + (int64_t)cout * hd + hd + cout;
}

template <typename T> struct WArgs {
  const T *x, *dy, *w1, *w2t, *b1;   // w2t: W2^T [hd, cout]
  float *partial;                     // [splits * 4][image_floats]
  int64_t n;
  int c, hd, cout, act, splits;
};

// LDS: [32][c + PAD] (W1 chunk), [32][cout + PAD] (W2^T chunk), four wave-private [max(c, cout)][32 + PAD] transposed images
static inline int64_t w_lds_bytes(int elem, int c, int cout) {
  const int pad = 16 / elem;
  return ((int64_t)32 * (c + pad) + 32 * (cout + pad) + 4 * (int64_t)std::max(c, cout) * (32 + pad)) * elem;
}

template <typename T, int MT> __global__ __launch_bounds__(kThreads) void k_ffn_bwd_w(const WArgs<T> a) {
  constexpr int PAD = FfnT<T>::PAD;
  extern __shared__ __attribute__((aligned(16))) unsigned char s_ffn[];
  const int c = a.c, hd = a.hd, cout = a.cout;
  const int lda = c + PAD, ldb = cout + PAD, ldt = 32 + PAD;
  const int nka = c / 16, nkb = cout / 16, ntc = c / 32, nto = cout / 32;
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, r = lane & 31, h = lane >> 5;
  const int j = blockIdx.x, split = blockIdx.y;
  T *s_w1 = reinterpret_cast<T *>(s_ffn), *s_w2t = s_w1 + 32 * lda;
  T *s_t = s_w2t + 32 * ldb + wave * (c > cout ? c : cout) * ldt;
  stage<T>(a.w1 + (int64_t)32 * j * c, c, 32, c, s_w1, lda);
  stage<T>(a.w2t + (int64_t)32 * j * cout, cout, 32, cout, s_w2t, ldb);
  float bias[16];
  {
    const float b = a.b1 != nullptr ? (float)a.b1[32 * j + r] : 0.f;   // the hidden unit is the lane
#pragma unroll
    for (int i = 0; i < 16; ++i) bias[i] = b;
  }
  ff_f32x16 dw1[MT], dw2[MT];
#pragma unroll
  for (int t = 0; t < MT; ++t) { ffn_zero(dw1[t]); ffn_zero(dw2[t]); }
  float db1 = 0.f, db2[MT / 2];
#pragma unroll
  for (int q = 0; q < MT / 2; ++q) db2[q] = 0.f;

  const int64_t blocks = (a.n + kRows - 1) / kRows, per = (blocks + a.splits - 1) / a.splits;
  const int64_t blk_end = (split + 1) * per < blocks ? (split + 1) * per : blocks;
  __syncthreads();
  for (int64_t blk = split * per; blk < blk_end; ++blk) {   // workgroup-uniform
    const int64_t row = blk * kRows + wave * 32 + r, rc = row < a.n ? row : a.n - 1;
    const bool valid = row < a.n;
    ff_f32x16 z, dh;
    ffn_zero(z);
    ffn_zero(dh);
#pragma unroll
    for (int k = 0; k < 2 * MT; ++k) {
      if (k >= nka) continue;
      const Frag<T> xa = valid ? ffn_load8(a.x + rc * c + 16 * k + 8 * h) : ffn_zero_frag<T>();
      ffn_mma(z, xa, ffn_load8(s_w1 + r * lda + 16 * k + 8 * h));   // Z[row][hidden]
      scatter_t<T>(s_t, ldt, 16 * k + 8 * h, r, xa);
    }
#pragma unroll
    for (int k = 0; k < 2 * MT; ++k) {
      if (k >= nkb) continue;
      const Frag<T> ga = valid ? ffn_load8(a.dy + rc * cout + 16 * k + 8 * h) : ffn_zero_frag<T>();
      ffn_mma(dh, ga, ffn_load8(s_w2t + r * ldb + 16 * k + 8 * h));   // dH[row][hidden]
    }
    float dz[16], hact[16];
    hidden<true>(a.act, z, dh, bias, dz, hact);
#pragma unroll
    for (int i = 0; i < 16; ++i) db1 += dz[i];   // a clamped row has dh = 0
    __syncthreads();   // X^T is in the wave's image
#pragma unroll
    for (int s = 0; s < 2; ++s) {
      const Frag<T> f = ffn_acc_frag<T>(dz, s);
#pragma unroll
      for (int t = 0; t < MT; ++t)   // dW1^T[channel][hidden] += X^T[channel][row] dZ[row][hidden]
        if (t < ntc) ffn_mma(dw1[t], ffn_load44(s_t + (t * 32 + r) * ldt + 16 * s + 4 * h), f);
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < 2 * MT; ++k) {
      if (k >= nkb) continue;
      const Frag<T> ga = valid ? ffn_load8(a.dy + rc * cout + 16 * k + 8 * h) : ffn_zero_frag<T>();
      scatter_t<T>(s_t, ldt, 16 * k + 8 * h, r, ga);
    }
    __syncthreads();   // dY^T is in the wave's image
#pragma unroll
    for (int s = 0; s < 2; ++s) {
      const Frag<T> f = ffn_acc_frag<T>(hact, s);
#pragma unroll
      for (int t = 0; t < MT; ++t)   // dW2[channel][hidden] += dY^T[channel][row] H[row][hidden]
        if (t < nto) ffn_mma(dw2[t], ffn_load44(s_t + (t * 32 + r) * ldt + 16 * s + 4 * h), f);
    }
    if (j == 0) {   // db2: a lane sums the 32 rows of its channels in ascending order
#pragma unroll
      for (int q = 0; q < MT / 2; ++q) {
        const int ch = lane + 64 * q;
        if (ch < cout)
          for (int k = 0; k < 32; ++k) db2[q] += (float)s_t[ch * ldt + k];
      }
    }
    __syncthreads();   // the image is free for the next step
  }

  float *img = a.partial + ((int64_t)split * 4 + wave) * image_floats(c, hd, cout);
#pragma unroll
  for (int t = 0; t < MT; ++t) {
    if (t >= ntc) continue;
#pragma unroll
    for (int g = 0; g < 4; ++g)
      ffn_store4(img + (int64_t)(32 * j + r) * c + 32 * t + 8 * g + 4 * h, dw1[t][4 * g], dw1[t][4 * g + 1],
                 dw1[t][4 * g + 2], dw1[t][4 * g + 3]);
  }
  img += (int64_t)hd * c;
#pragma unroll
  for (int t = 0; t < MT; ++t) {
    if (t >= nto) continue;
#pragma unroll
    for (int i = 0; i < 16; ++i) img[(int64_t)(32 * t + ffn_row(i, h)) * hd + 32 * j + r] = dw2[t][i];
  }
  img += (int64_t)cout * hd;
  const float other = __shfl_xor(db1, 32, 64);
  if (h == 0) img[32 * j + r] = db1 + other;
  if (j == 0) {
    img += hd;
#pragma unroll
    for (int q = 0; q < MT / 2; ++q)
      if (lane + 64 * q < cout) img[lane + 64 * q] = db2[q];
  }
}

// element e of the image: the sum of the `slots` partial images in ascending order, rounded once to T.  A null destination
// is not written.
template <typename T>
__global__ __launch_bounds__(kThreads) void k_ffn_reduce(const float *__restrict__ partial, int slots, int c, int hd,
                                                         int cout, T *__restrict__ dw1, T *__restrict__ db1,
                                                         T *__restrict__ dw2, T *__restrict__ db2) {
  const int64_t total = image_floats(c, hd, cout), e = (int64_t)blockIdx.x * kThreads + threadIdx.x;
  if (e >= total) return;
  const int64_t n1 = (int64_t)hd * c, n2 = n1 + (int64_t)cout * hd, n3 = n2 + hd;
  T *dst = e < n1 ? (dw1 ? dw1 + e : nullptr)
                  : e < n2 ? (dw2 ? dw2 + (e - n1) : nullptr)
                           : e < n3 ? (db1 ? db1 + (e - n2) : nullptr) : (db2 ? db2 + (e - n3) : nullptr);
  if (dst == nullptr) return;
  float s = 0.f;
  for (int q = 0; q < slots; ++q) s += partial[q * total + e];
  *dst = (T)s;
}

// ---- host side: the family description of feed_forward.hpp's launch and policy code ---------------------------------------
struct Plain {
  static constexpr int NZ = 1, kMaxBf16 = ME_FFN_MAX_WIDTH_BF16, kMaxF32 = ME_FFN_MAX_WIDTH_F32;
  template <typename T> using Rows = RowsArgs<T>;
  template <typename T> using Weights = WArgs<T>;
  template <typename T, int MT> static auto fwd() { return &k_ffn_fwd<T, MT>; }
  template <typename T, int MT> static auto bwd_x() { return &k_ffn_bwd_x<T, MT>; }
  template <typename T, int MT> static auto bwd_w() { return &k_ffn_bwd_w<T, MT>; }
  static int64_t rows_lds(int elem, int c, int cout, bool bwd) { return rows_lds_bytes(elem, c, cout, bwd); }
  static int64_t w_lds(int elem, int c, int cout) { return w_lds_bytes(elem, c, cout); }
  static int64_t image(int c, int hd, int cout) { return image_floats(c, hd, cout); }
  // wt = {W1^T}, w2t: backward (out = dx); null: forward (out = y)
  template <typename T> static Rows<T> rows(const Call<1> &m, T *const *wt, T *w2t) {
    if (wt == nullptr)
      return {(const T *)m.x, nullptr, (const T *)m.w[0], nullptr, (const T *)m.w2, (const T *)m.b[0], (const T *)m.b2,
              (T *)m.out, m.n, m.c, m.hd, m.cout, m.act};
    return {(const T *)m.x, (const T *)m.dy, (const T *)m.w[0], w2t, wt[0], (const T *)m.b[0], nullptr, (T *)m.out, m.n,
            m.c, m.hd, m.cout, m.act};
  }
  template <typename T> static Weights<T> weights(const Call<1> &m, T *w2t, float *partial, int splits) {
    return {(const T *)m.x, (const T *)m.dy, (const T *)m.w[0], w2t, (const T *)m.b[0], partial, m.n, m.c, m.hd, m.cout,
            m.act, splits};
  }
  template <typename T> static void reduce(const Call<1> &m, const float *partial, int slots, hipStream_t stream) {
    hipLaunchKernelGGL(k_ffn_reduce<T>, dim3((unsigned)ceil_div(image_floats(m.c, m.hd, m.cout), kThreads)), dim3(kThreads),
                       0, stream, partial, slots, m.c, m.hd, m.cout, (T *)m.dw[0], (T *)m.db[0], (T *)m.dw2, (T *)m.db2);
  }
};

}  // namespace ffn
}  // namespace me

using namespace me;
using namespace me::ffn;

extern "C" {

int32_t me_ffn_supported(int32_t c, int32_t hd, int32_t cout, int32_t elem_bytes) {
  return supported<Plain>(c, hd, cout, elem_bytes);
}

int32_t me_ffn_row_splits(int64_t n, int32_t c, int32_t hd, int32_t cout, int32_t elem_bytes) {
  return row_splits<Plain>(n, c, hd, cout, elem_bytes);
}

int64_t me_ffn_workspace_bytes(int64_t n, int32_t c, int32_t hd, int32_t cout, int32_t elem_bytes) {
  return workspace_bytes<Plain>(n, c, hd, cout, elem_bytes);
}

int me_ffn_forward(const void *x_dev, const void *w1_dev, const void *b1_dev, const void *w2_dev, const void *b2_dev,
                   int32_t is_bf16, int64_t n, int32_t c, int32_t hd, int32_t cout, int32_t activation, void *y_dev,
                   void *stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  ME_FFN_CHECK_SHAPE(Plain, "ME_FFN_MAX_WIDTH", n, c, hd, cout, is_bf16 ? 2 : 4, activation);
  if (n == 0) return 0;
  ME_CHECK(x_dev != nullptr && w1_dev != nullptr && w2_dev != nullptr && y_dev != nullptr, "x, w1, w2 and y must be given");
  ME_CHECK(aligned16({x_dev, w1_dev, w2_dev, y_dev}), "x, w1, w2 and y must be aligned to 16 bytes");
  Call<1> m{};
  m.x = x_dev, m.w[0] = w1_dev, m.b[0] = b1_dev, m.w2 = w2_dev, m.b2 = b2_dev, m.out = y_dev;
  m.n = n, m.c = c, m.hd = hd, m.cout = cout, m.act = activation;
  return is_bf16 ? forward<Plain, __bf16>(m, stream) : forward<Plain, float>(m, stream);
}

int me_ffn_backward(const void *x_dev, const void *dy_dev, const void *w1_dev, const void *b1_dev, const void *w2_dev,
                    int32_t is_bf16, int64_t n, int32_t c, int32_t hd, int32_t cout, int32_t activation,
                    int32_t need_dx, int32_t need_fc1, int32_t need_fc2, void *dx_dev, void *dw1_dev, void *db1_dev,
                    void *dw2_dev, void *db2_dev, void *workspace_dev, int64_t workspace_bytes, void *stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  const int elem = is_bf16 ? 2 : 4;
  ME_FFN_CHECK_SHAPE(Plain, "ME_FFN_MAX_WIDTH", n, c, hd, cout, elem, activation);
  ME_CHECK(!need_dx || dx_dev != nullptr, "need_dx without dx");
  ME_CHECK(!need_fc1 || dw1_dev != nullptr, "need_fc1 without dw1");
  ME_CHECK(!need_fc2 || dw2_dev != nullptr, "need_fc2 without dw2");
  const bool need_w = need_fc1 != 0 || need_fc2 != 0;
  if (!need_dx && !need_w) return 0;
  // n = 0: the reduce over the images of one empty split writes the zeros
  ME_CHECK(workspace_dev != nullptr && workspace_bytes >= me_ffn_workspace_bytes(n, c, hd, cout, elem),
           "the workspace must hold me_ffn_workspace_bytes");
  ME_CHECK(w1_dev != nullptr && w2_dev != nullptr && (n == 0 || (x_dev != nullptr && dy_dev != nullptr)),
           "x, dy, w1 and w2 must be given");
  ME_CHECK(aligned16({x_dev, dy_dev, w1_dev, w2_dev, dx_dev, workspace_dev}), "the operands must be aligned to 16 bytes");
  Call<1> m{};
  m.x = x_dev, m.dy = dy_dev, m.w[0] = w1_dev, m.b[0] = b1_dev, m.w2 = w2_dev, m.out = dx_dev, m.ws = workspace_dev;
  if (need_fc1) m.dw[0] = dw1_dev, m.db[0] = db1_dev;
  if (need_fc2) m.dw2 = dw2_dev, m.db2 = db2_dev;
  m.n = n, m.c = c, m.hd = hd, m.cout = cout, m.act = activation, m.need_dx = need_dx != 0 && n > 0, m.need_w = need_w;
  return is_bf16 ? backward<Plain, __bf16>(m, stream) : backward<Plain, float>(m, stream);
}

}  // extern "C"
