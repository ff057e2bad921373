// Fused gated MLP (SwiGLU / GeGLU / ReGLU) over the rows of a feature matrix for gfx950 (MI355X):
//   y = (act(x Wg^T + bg) * (x Wu^T + bu)) W2^T + b2
// with x [n, C], Wg and Wu [Hd, C], W2 [Cout, Hd] (torch.nn.Linear's layouts).  None of the three [n, Hd] matrices of the
// unfused form (gate, up, product) reaches memory, in either direction: every kernel recomputes the 32-wide chunk of them
// that it needs from x.  The design is that of feed_forward.hip, whose fragment helpers it shares (feed_forward.hpp), with
// a second first product off the same x fragments:
//
//   k_glu_fwd     row-stationary.  A workgroup of four waves owns 128 rows, a wave 32 of them; the wave's rows of x stay in
//                 registers as B fragments.  Per chunk: Zg^T = Wg[chunk, :] X^T and Zu^T = Wu[chunk, :] X^T (every x
//                 fragment feeds two MFMAs), H = act(Zg + bg) (Zu + bu) in fp32 registers, Y^T += W2[:, chunk] H^T with the
//                 16 registers of H as the two k-steps of the B operand (ffn_acc_frag / ffn_load44).
//   k_glu_bwd_x   the same body: Zg, Zu recomputed, dH^T = W2^T[chunk, :] dY^T, dZg = dH (Zu + bu) act'(Zg + bg),
//                 dZu = dH act(Zg + bg), dX^T += Wg^T[:, chunk] dZg^T + Wu^T[:, chunk] dZu^T: two second products into one
//                 accumulator set.  The three transposed weights come from k_ffn_transpose (once per backward call).
//   k_glu_bwd_w   hidden-stationary.  A workgroup owns (32-wide hidden chunk, row split) and walks its rows 128 at a time,
//                 a wave 32 of them; the products are taken plain (the hidden unit on the lane), dWg[chunk, :],
//                 dWu[chunk, :], dW2[:, chunk], dbg[chunk] and dbu[chunk] of the wave's rows stay in registers and are
//                 written once as an fp32 partial image per (split, wave).  db2 rides in the chunk-0 workgroups.
//   k_glu_reduce  sums the partial images in ascending (split, wave) order and rounds once to the parameter type.
//
// bf16 rows: H, dZg and dZu are rounded once where they become an MFMA operand; fp32 rows stay fp32 on the exact
// 32x32x2 MFMA; all accumulation is fp32; outputs are rounded once.  No atomics, fixed summation orders: bitwise reproducible.
// The weight blocks of a chunk are staged in 16-byte pieces, double-buffered in the row-stationary kernels (one barrier per
// chunk).  A partial last row block clamps the row index and masks the store (the weight-gradient kernel zeroes the clamped
// rows of x and dy instead).
// Widths: C and Cout multiples of 32 up to ME_GLU_MAX_WIDTH_BF16 / ME_GLU_MAX_WIDTH_F32, Hd any multiple of 32; one
// instantiation per (dtype, MT) with MT = 2 | 4 (bf16) or 2 (fp32) register tiles for max(C, Cout) / 32.
#include "feed_forward.hpp"

namespace me {
namespace glu {

using namespace me::ffn;

constexpr int kBiasBytes = 2 * 2 * 32 * (int)sizeof(float);   // [buffer][gate | up][32]

// H = act(zg + bg) (zu + bu).  GRAD: also dzg = dh (zu + bu) act'(zg + bg) and dzu = dh act(zg + bg).
template <int A, bool GRAD>
__device__ __forceinline__ void gated_one(const ff_f32x16 &zg, const ff_f32x16 &zu, const ff_f32x16 &dh,
                                          const float (&bg)[16], const float (&bu)[16], float (&hv)[16],
                                          float (&dzg)[16], float (&dzu)[16]) {
#pragma unroll
  for (int i = 0; i < 16; ++i) {
    const float g = zg[i] + bg[i], u = zu[i] + bu[i], a = act_f<A>(g);
    hv[i] = a * u;
    if constexpr (GRAD) {
      dzg[i] = dh[i] * u * act_g<A>(g);
      dzu[i] = dh[i] * a;
    }
  }
}
template <bool GRAD>
__device__ __forceinline__ void gated(int act, const ff_f32x16 &zg, const ff_f32x16 &zu, const ff_f32x16 &dh,
                                      const float (&bg)[16], const float (&bu)[16], float (&hv)[16], float (&dzg)[16],
                                      float (&dzu)[16]) {
  switch (act) {   // wave-uniform
    case ME_FFN_RELU: gated_one<ME_FFN_RELU, GRAD>(zg, zu, dh, bg, bu, hv, dzg, dzu); break;
    case ME_FFN_GELU: gated_one<ME_FFN_GELU, GRAD>(zg, zu, dh, bg, bu, hv, dzg, dzu); break;
    case ME_FFN_GELU_TANH: gated_one<ME_FFN_GELU_TANH, GRAD>(zg, zu, dh, bg, bu, hv, dzg, dzu); break;
    default: gated_one<ME_FFN_SILU, GRAD>(zg, zu, dh, bg, bu, hv, dzg, dzu); break;
  }
}

// ---- row-stationary: forward and input gradient ----------------------------------------------------------------------
// forward:  x, wg, wu [hd, c], w2 [cout, hd], bg, bu, b2 -> out = y [n, cout]
// backward: x, g = dy [n, cout], wg, wu, w2t = W2^T [hd, cout], wgt = Wg^T and wut = Wu^T [c, hd], bg, bu -> out = dx [n, c]
template <typename T> struct RowsArgs {
  const T *x, *g, *wg, *wu, *w2, *w2t, *wgt, *wut, *bg, *bu, *b2;
  T *out;
  int64_t n;
  int c, hd, cout, act;
};

// LDS: the bias chunks, then two buffers of 2 x [32][c + PAD] (wg, wu) and
//   forward:  [cout][32 + PAD] (w2)        backward: [32][cout + PAD] (w2t), 2 x [c][32 + PAD] (wgt, wut)
static inline int64_t rows_lds_bytes(int elem, int c, int cout, bool bwd) {
  const int pad = 16 / elem;
  const int64_t buf = 2 * 32 * (c + pad) + (bwd ? 32 * (cout + pad) + 2 * (int64_t)c * (32 + pad) : (int64_t)cout * (32 + pad));
  return kBiasBytes + 2 * buf * elem;
}

template <typename T, int MT, bool BWD> __device__ __forceinline__ void glu_rows(const RowsArgs<T> &a) {
  constexpr int PAD = FfnT<T>::PAD;
  extern __shared__ __attribute__((aligned(16))) unsigned char s_glu[];
  float *s_bias = reinterpret_cast<float *>(s_glu);   // [2][2][32]
  T *s_buf = reinterpret_cast<T *>(s_glu + kBiasBytes);
  const int c = a.c, hd = a.hd, cout = a.cout, co = BWD ? c : cout;
  const int lda = c + PAD, ldb = cout + PAD, ldc = 32 + PAD;
  // offsets in a buffer: wg 0, wu 32 lda, then (forward) w2 | (backward) w2t, wgt, wut
  const int off_b = 2 * 32 * lda, off_c = off_b + (BWD ? 32 * ldb : 0), off_d = off_c + co * ldc;
  const int buf_elems = off_d + (BWD ? co * ldc : 0);
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
    T *s = s_buf + (j & 1) * buf_elems;
    stage<T>(a.wg + (int64_t)32 * j * c, c, 32, c, s, lda);
    stage<T>(a.wu + (int64_t)32 * j * c, c, 32, c, s + 32 * lda, lda);
    if constexpr (BWD) {
      stage<T>(a.w2t + (int64_t)32 * j * cout, cout, 32, cout, s + off_b, ldb);
      stage<T>(a.wgt + 32 * j, hd, c, 32, s + off_c, ldc);
      stage<T>(a.wut + 32 * j, hd, c, 32, s + off_d, ldc);
    } else {
      stage<T>(a.w2 + 32 * j, hd, cout, 32, s + off_c, ldc);
    }
    if (threadIdx.x < 64) {
      const T *b = threadIdx.x < 32 ? a.bg : a.bu;
      s_bias[(j & 1) * 64 + threadIdx.x] = b != nullptr ? (float)b[32 * j + (threadIdx.x & 31)] : 0.f;
    }
  };
  stage_chunk(0);
  for (int j = 0; j < nchunks; ++j) {
    __syncthreads();   // chunk j is staged, and every wave is done with chunk j - 1, whose buffer chunk j + 1 takes
    if (j + 1 < nchunks) stage_chunk(j + 1);
    const T *s = s_buf + (j & 1) * buf_elems;
    ff_f32x16 zg, zu;
    ffn_zero(zg);
    ffn_zero(zu);
#pragma unroll
    for (int k = 0; k < 2 * MT; ++k) {
      if (k >= nka) continue;
      ffn_mma(zg, ffn_load8(s + r * lda + 16 * k + 8 * h), xf[k]);               // Zg^T[hidden][row]
      ffn_mma(zu, ffn_load8(s + (32 + r) * lda + 16 * k + 8 * h), xf[k]);        // Zu^T[hidden][row]
    }
    float bg[16], bu[16], hv[16], dzg[16], dzu[16];
#pragma unroll
    for (int i = 0; i < 16; ++i) {
      bg[i] = s_bias[(j & 1) * 64 + ffn_row(i, h)];
      bu[i] = s_bias[(j & 1) * 64 + 32 + ffn_row(i, h)];
    }
    if constexpr (BWD) {
      ff_f32x16 dh;
      ffn_zero(dh);
#pragma unroll
      for (int k = 0; k < 2 * MT; ++k)
        if (k < nkb) ffn_mma(dh, ffn_load8(s + off_b + r * ldb + 16 * k + 8 * h), gf[k]);   // dH^T[hidden][row]
      gated<true>(a.act, zg, zu, dh, bg, bu, hv, dzg, dzu);
#pragma unroll
      for (int q = 0; q < 2; ++q) {
        const Frag<T> fg = ffn_acc_frag<T>(dzg, q), fu = ffn_acc_frag<T>(dzu, q);
#pragma unroll
        for (int t = 0; t < MT; ++t) {   // dX^T[channel][row] += Wg^T[channel][hidden] dZg^T + Wu^T[channel][hidden] dZu^T
          if (t >= nto) continue;
          ffn_mma(o[t], ffn_load44(s + off_c + (t * 32 + r) * ldc + 16 * q + 4 * h), fg);
          ffn_mma(o[t], ffn_load44(s + off_d + (t * 32 + r) * ldc + 16 * q + 4 * h), fu);
        }
      }
    } else {
      gated<false>(a.act, zg, zu, zg, bg, bu, hv, dzg, dzu);
#pragma unroll
      for (int q = 0; q < 2; ++q) {
        const Frag<T> hf = ffn_acc_frag<T>(hv, q);
#pragma unroll
        for (int t = 0; t < MT; ++t)   // Y^T[channel][row] += W2[channel][hidden] H^T[hidden][row]
          if (t < nto) ffn_mma(o[t], ffn_load44(s + off_c + (t * 32 + r) * ldc + 16 * q + 4 * h), hf);
      }
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

template <typename T, int MT> __global__ __launch_bounds__(kThreads) void k_glu_fwd(const RowsArgs<T> a) {
  glu_rows<T, MT, false>(a);
}
template <typename T, int MT> __global__ __launch_bounds__(kThreads) void k_glu_bwd_x(const RowsArgs<T> a) {
  glu_rows<T, MT, true>(a);
}

// ---- weight gradient: hidden-stationary -------------------------------------------------------------------------------
// floats of one partial image: [dWg hd x c | dWu hd x c | dW2 cout x hd | dbg hd | dbu hd | db2 cout]
static __host__ __device__ __forceinline__ int64_t image_floats(int c, int hd, int cout) {
  return 2 * (int64_t)hd * c + (int64_t)cout * hd + 2 * hd + cout;
}

template <typename T> struct WArgs {
  const T *x, *dy, *wg, *wu, *w2t, *bg, *bu;   // w2t: W2^T [hd, cout]
  float *partial;                               // [splits * 4][image_floats]
  int64_t n;
  int c, hd, cout, act, splits;
};

// LDS: 2 x [32][c + PAD] (Wg, Wu chunks), [32][cout + PAD] (W2^T chunk), four wave-private [max(c, cout)][32 + PAD]
// transposed images
static inline int64_t w_lds_bytes(int elem, int c, int cout) {
  const int pad = 16 / elem;
  return ((int64_t)2 * 32 * (c + pad) + 32 * (cout + pad) + 4 * (int64_t)std::max(c, cout) * (32 + pad)) * elem;
}

template <typename T, int MT> __global__ __launch_bounds__(kThreads) void k_glu_bwd_w(const WArgs<T> a) {
  constexpr int PAD = FfnT<T>::PAD;
  extern __shared__ __attribute__((aligned(16))) unsigned char s_glu[];
  const int c = a.c, hd = a.hd, cout = a.cout;
  const int lda = c + PAD, ldb = cout + PAD, ldt = 32 + PAD;
  const int nka = c / 16, nkb = cout / 16, ntc = c / 32, nto = cout / 32;
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, r = lane & 31, h = lane >> 5;
  const int j = blockIdx.x, split = blockIdx.y;
  T *s_wg = reinterpret_cast<T *>(s_glu), *s_wu = s_wg + 32 * lda, *s_w2t = s_wu + 32 * lda;
  T *s_t = s_w2t + 32 * ldb + wave * (c > cout ? c : cout) * ldt;
  stage<T>(a.wg + (int64_t)32 * j * c, c, 32, c, s_wg, lda);
  stage<T>(a.wu + (int64_t)32 * j * c, c, 32, c, s_wu, lda);
  stage<T>(a.w2t + (int64_t)32 * j * cout, cout, 32, cout, s_w2t, ldb);
  float bg[16], bu[16];
  {
    const float g = a.bg != nullptr ? (float)a.bg[32 * j + r] : 0.f;   // the hidden unit is the lane
    const float u = a.bu != nullptr ? (float)a.bu[32 * j + r] : 0.f;
#pragma unroll
    for (int i = 0; i < 16; ++i) { bg[i] = g; bu[i] = u; }
  }
  ff_f32x16 dwg[MT], dwu[MT], dw2[MT];
#pragma unroll
  for (int t = 0; t < MT; ++t) { ffn_zero(dwg[t]); ffn_zero(dwu[t]); ffn_zero(dw2[t]); }
  float dbg = 0.f, dbu = 0.f, db2[MT / 2];
#pragma unroll
  for (int q = 0; q < MT / 2; ++q) db2[q] = 0.f;

  const int64_t blocks = (a.n + kRows - 1) / kRows, per = (blocks + a.splits - 1) / a.splits;
  const int64_t blk_end = (split + 1) * per < blocks ? (split + 1) * per : blocks;
  __syncthreads();
  for (int64_t blk = split * per; blk < blk_end; ++blk) {   // workgroup-uniform
    const int64_t row = blk * kRows + wave * 32 + r, rc = row < a.n ? row : a.n - 1;
    const bool valid = row < a.n;
    ff_f32x16 zg, zu, dh;
    ffn_zero(zg);
    ffn_zero(zu);
    ffn_zero(dh);
#pragma unroll
    for (int k = 0; k < 2 * MT; ++k) {
      if (k >= nka) continue;
      const Frag<T> xa = valid ? ffn_load8(a.x + rc * c + 16 * k + 8 * h) : ffn_zero_frag<T>();
      ffn_mma(zg, xa, ffn_load8(s_wg + r * lda + 16 * k + 8 * h));   // Zg[row][hidden]
      ffn_mma(zu, xa, ffn_load8(s_wu + r * lda + 16 * k + 8 * h));   // Zu[row][hidden]
      scatter_t<T>(s_t, ldt, 16 * k + 8 * h, r, xa);
    }
#pragma unroll
    for (int k = 0; k < 2 * MT; ++k) {
      if (k >= nkb) continue;
      const Frag<T> ga = valid ? ffn_load8(a.dy + rc * cout + 16 * k + 8 * h) : ffn_zero_frag<T>();
      ffn_mma(dh, ga, ffn_load8(s_w2t + r * ldb + 16 * k + 8 * h));   // dH[row][hidden]
    }
    float hv[16], dzg[16], dzu[16];
    gated<true>(a.act, zg, zu, dh, bg, bu, hv, dzg, dzu);
#pragma unroll
    for (int i = 0; i < 16; ++i) { dbg += dzg[i]; dbu += dzu[i]; }   // a clamped row has dh = 0
    __syncthreads();   // X^T is in the wave's image
#pragma unroll
    for (int q = 0; q < 2; ++q) {
      const Frag<T> fg = ffn_acc_frag<T>(dzg, q), fu = ffn_acc_frag<T>(dzu, q);
#pragma unroll
      for (int t = 0; t < MT; ++t) {   // dWg^T[channel][hidden] += X^T[channel][row] dZg[row][hidden]; dWu alike
        if (t >= ntc) continue;
        const Frag<T> xt = ffn_load44(s_t + (t * 32 + r) * ldt + 16 * q + 4 * h);
        ffn_mma(dwg[t], xt, fg);
        ffn_mma(dwu[t], xt, fu);
      }
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
    for (int q = 0; q < 2; ++q) {
      const Frag<T> f = ffn_acc_frag<T>(hv, q);
#pragma unroll
      for (int t = 0; t < MT; ++t)   // dW2[channel][hidden] += dY^T[channel][row] H[row][hidden]
        if (t < nto) ffn_mma(dw2[t], ffn_load44(s_t + (t * 32 + r) * ldt + 16 * q + 4 * h), f);
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
  for (int m = 0; m < 2; ++m) {   // dWg, then dWu
#pragma unroll
    for (int t = 0; t < MT; ++t) {
      if (t >= ntc) continue;
      const ff_f32x16 &d = m == 0 ? dwg[t] : dwu[t];
#pragma unroll
      for (int g = 0; g < 4; ++g)
        ffn_store4(img + (int64_t)(32 * j + r) * c + 32 * t + 8 * g + 4 * h, d[4 * g], d[4 * g + 1], d[4 * g + 2],
                   d[4 * g + 3]);
    }
    img += (int64_t)hd * c;
  }
#pragma unroll
  for (int t = 0; t < MT; ++t) {
    if (t >= nto) continue;
#pragma unroll
    for (int i = 0; i < 16; ++i) img[(int64_t)(32 * t + ffn_row(i, h)) * hd + 32 * j + r] = dw2[t][i];
  }
  img += (int64_t)cout * hd;
  const float og = __shfl_xor(dbg, 32, 64), ou = __shfl_xor(dbu, 32, 64);
  if (h == 0) {
    img[32 * j + r] = dbg + og;
    img[hd + 32 * j + r] = dbu + ou;
  }
  if (j == 0) {
    img += 2 * hd;
#pragma unroll
    for (int q = 0; q < MT / 2; ++q)
      if (lane + 64 * q < cout) img[lane + 64 * q] = db2[q];
  }
}

// destinations of the reduce, in the order of the image; a null one is not written
template <typename T> struct Grads {
  T *dwg, *dwu, *dw2, *dbg, *dbu, *db2;
};

// element e of the image: the sum of the `slots` partial images in ascending order, rounded once to T
template <typename T>
__global__ __launch_bounds__(kThreads) void k_glu_reduce(const float *__restrict__ partial, int slots, int c, int hd,
                                                         int cout, const Grads<T> g) {
  const int64_t total = image_floats(c, hd, cout), e = (int64_t)blockIdx.x * kThreads + threadIdx.x;
  if (e >= total) return;
  const int64_t n1 = (int64_t)hd * c, n2 = 2 * n1, n3 = n2 + (int64_t)cout * hd, n4 = n3 + hd, n5 = n4 + hd;
  T *base = e < n1 ? g.dwg : e < n2 ? g.dwu : e < n3 ? g.dw2 : e < n4 ? g.dbg : e < n5 ? g.dbu : g.db2;
  const int64_t first = e < n1 ? 0 : e < n2 ? n1 : e < n3 ? n2 : e < n4 ? n3 : e < n5 ? n4 : n5;
  if (base == nullptr) return;
  float s = 0.f;
  for (int q = 0; q < slots; ++q) s += partial[q * total + e];
  base[e - first] = (T)s;
}

// ---- host side: the family description of feed_forward.hpp's launch and policy code ---------------------------------------
struct Gated {
  static constexpr int NZ = 2, kMaxBf16 = ME_GLU_MAX_WIDTH_BF16, kMaxF32 = ME_GLU_MAX_WIDTH_F32;
  template <typename T> using Rows = RowsArgs<T>;
  template <typename T> using Weights = WArgs<T>;
  template <typename T, int MT> static auto fwd() { return &k_glu_fwd<T, MT>; }
  template <typename T, int MT> static auto bwd_x() { return &k_glu_bwd_x<T, MT>; }
  template <typename T, int MT> static auto bwd_w() { return &k_glu_bwd_w<T, MT>; }
  static int64_t rows_lds(int elem, int c, int cout, bool bwd) { return rows_lds_bytes(elem, c, cout, bwd); }
  static int64_t w_lds(int elem, int c, int cout) { return w_lds_bytes(elem, c, cout); }
  static int64_t image(int c, int hd, int cout) { return image_floats(c, hd, cout); }
  // wt = {Wg^T, Wu^T}, w2t: backward (out = dx); null: forward (out = y)
  template <typename T> static Rows<T> rows(const Call<2> &m, T *const *wt, T *w2t) {
    const bool bwd = wt != nullptr;
    return {(const T *)m.x, bwd ? (const T *)m.dy : nullptr, (const T *)m.w[0], (const T *)m.w[1],
            bwd ? nullptr : (const T *)m.w2, w2t, bwd ? wt[0] : nullptr, bwd ? wt[1] : nullptr, (const T *)m.b[0],
            (const T *)m.b[1], bwd ? nullptr : (const T *)m.b2, (T *)m.out, m.n, m.c, m.hd, m.cout, m.act};
  }
  template <typename T> static Weights<T> weights(const Call<2> &m, T *w2t, float *partial, int splits) {
    return {(const T *)m.x, (const T *)m.dy, (const T *)m.w[0], (const T *)m.w[1], w2t, (const T *)m.b[0],
            (const T *)m.b[1], partial, m.n, m.c, m.hd, m.cout, m.act, splits};
  }
  template <typename T> static void reduce(const Call<2> &m, const float *partial, int slots, hipStream_t stream) {
    const Grads<T> g{(T *)m.dw[0], (T *)m.dw[1], (T *)m.dw2, (T *)m.db[0], (T *)m.db[1], (T *)m.db2};
    hipLaunchKernelGGL(k_glu_reduce<T>, dim3((unsigned)ceil_div(image_floats(m.c, m.hd, m.cout), kThreads)), dim3(kThreads),
                       0, stream, partial, slots, m.c, m.hd, m.cout, g);
  }
};

}  // namespace glu
}  // namespace me

using namespace me;
using namespace me::glu;

extern "C" {

int32_t me_glu_supported(int32_t c, int32_t hd, int32_t cout, int32_t elem_bytes) {
  return supported<Gated>(c, hd, cout, elem_bytes);
}

int32_t me_glu_row_splits(int64_t n, int32_t c, int32_t hd, int32_t cout, int32_t elem_bytes) {
  return row_splits<Gated>(n, c, hd, cout, elem_bytes);
}

int64_t me_glu_workspace_bytes(int64_t n, int32_t c, int32_t hd, int32_t cout, int32_t elem_bytes) {
  return workspace_bytes<Gated>(n, c, hd, cout, elem_bytes);
}

int me_glu_forward(const void *x_dev, const void *wg_dev, const void *bg_dev, const void *wu_dev, const void *bu_dev,
                   const void *w2_dev, const void *b2_dev, int32_t is_bf16, int64_t n, int32_t c, int32_t hd,
                   int32_t cout, int32_t activation, void *y_dev, void *stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  ME_FFN_CHECK_SHAPE(Gated, "ME_GLU_MAX_WIDTH", n, c, hd, cout, is_bf16 ? 2 : 4, activation);
  if (n == 0) return 0;
  ME_CHECK(x_dev != nullptr && wg_dev != nullptr && wu_dev != nullptr && w2_dev != nullptr && y_dev != nullptr,
           "x, wg, wu, w2 and y must be given");
  ME_CHECK(aligned16({x_dev, wg_dev, wu_dev, w2_dev, y_dev}), "x, wg, wu, w2 and y must be aligned to 16 bytes");
  Call<2> m{};
  m.x = x_dev, m.w[0] = wg_dev, m.b[0] = bg_dev, m.w[1] = wu_dev, m.b[1] = bu_dev, m.w2 = w2_dev, m.b2 = b2_dev;
  m.out = y_dev, m.n = n, m.c = c, m.hd = hd, m.cout = cout, m.act = activation;
  return is_bf16 ? forward<Gated, __bf16>(m, stream) : forward<Gated, float>(m, stream);
}

int me_glu_backward(const void *x_dev, const void *dy_dev, const void *wg_dev, const void *bg_dev, const void *wu_dev,
                    const void *bu_dev, const void *w2_dev, int32_t is_bf16, int64_t n, int32_t c, int32_t hd,
                    int32_t cout, int32_t activation, int32_t need_dx, int32_t need_fc1, int32_t need_fc2, void *dx_dev,
                    void *dwg_dev, void *dbg_dev, void *dwu_dev, void *dbu_dev, void *dw2_dev, void *db2_dev,
                    void *workspace_dev, int64_t workspace_bytes, void *stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  const int elem = is_bf16 ? 2 : 4;
  ME_FFN_CHECK_SHAPE(Gated, "ME_GLU_MAX_WIDTH", n, c, hd, cout, elem, activation);
  ME_CHECK(!need_dx || dx_dev != nullptr, "need_dx without dx");
  ME_CHECK(!need_fc1 || (dwg_dev != nullptr && dwu_dev != nullptr), "need_fc1 without dwg and dwu");
  ME_CHECK(!need_fc2 || dw2_dev != nullptr, "need_fc2 without dw2");
  const bool need_w = need_fc1 != 0 || need_fc2 != 0;
  if (!need_dx && !need_w) return 0;
  // n = 0: the reduce over the images of one empty split writes the zeros
  ME_CHECK(workspace_dev != nullptr && workspace_bytes >= me_glu_workspace_bytes(n, c, hd, cout, elem),
           "the workspace must hold me_glu_workspace_bytes");
  ME_CHECK(wg_dev != nullptr && wu_dev != nullptr && w2_dev != nullptr && (n == 0 || (x_dev != nullptr && dy_dev != nullptr)),
           "x, dy, wg, wu and w2 must be given");
  ME_CHECK(aligned16({x_dev, dy_dev, wg_dev, wu_dev, w2_dev, dx_dev, workspace_dev}),
           "the operands must be aligned to 16 bytes");
  Call<2> m{};
  m.x = x_dev, m.dy = dy_dev, m.w[0] = wg_dev, m.b[0] = bg_dev, m.w[1] = wu_dev, m.b[1] = bu_dev, m.w2 = w2_dev;
  m.out = dx_dev, m.ws = workspace_dev;
  if (need_fc1) m.dw[0] = dwg_dev, m.db[0] = dbg_dev, m.dw[1] = dwu_dev, m.db[1] = dbu_dev;
  if (need_fc2) m.dw2 = dw2_dev, m.db2 = db2_dev;
  m.n = n, m.c = c, m.hd = hd, m.cout = cout, m.act = activation, m.need_dx = need_dx != 0 && n > 0, m.need_w = need_w;
  return is_bf16 ? backward<Gated, __bf16>(m, stream) : backward<Gated, float>(m, stream);
}

}  // extern "C"

// code-object preload (me_preload, coords.hip): resolving one kernel of this translation unit makes the runtime load the
// unit's whole code object now instead of at the first launch from it
extern "C" __attribute__((visibility("hidden"))) void me_preload_gated_feed_forward(void) {
  hipFuncAttributes attr;
  (void)hipFuncGetAttributes(&attr, reinterpret_cast<const void *>(&me::glu::k_glu_reduce<float>));
}
