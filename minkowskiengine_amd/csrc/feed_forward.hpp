// Fragment helpers of the fused MLP kernels for gfx950 (feed_forward.hip, gated_feed_forward.hip): the 32x32 MFMA shape of
// both dtypes, operand fragments and their loads from LDS, the accumulator-as-operand identity, the activations, the
// 16-byte staging of weight blocks and the weight transposition.
//
// One 32x32 MFMA shape serves both dtypes: v_mfma_f32_32x32x16_bf16 on bf16 rows, the exact v_mfma_f32_32x32x2_f32 on fp32
// rows; C/D lane map: column = lane & 31, row = (reg & 3) + 8 (reg >> 2) + 4 (lane >> 5).  The 16 accumulator registers of a
// tile are the two k-steps of the B operand of a following product with no lane movement: registers 8 s .. 8 s + 7 are
// k-step s, element j of lane half h being row 16 s + 8 (j >> 2) + 4 h + (j & 3); the A operand of that product is read in
// the same permuted k order (ffn_load44).
#pragma once
#include "common.hpp"

#include <initializer_list>

namespace me {
namespace ffn {

typedef float ff_f32x16 __attribute__((ext_vector_type(16)));
typedef float ff_f32x4 __attribute__((ext_vector_type(4)));
typedef __bf16 ff_bf16x8 __attribute__((ext_vector_type(8)));
typedef __bf16 ff_bf16x4 __attribute__((ext_vector_type(4)));

constexpr int kThreads = 256;            // four waves
constexpr int kRows = ME_FFN_ROWS;       // rows of a workgroup (step), 32 per wave
constexpr int kLdsBudget = 160 * 1024;
constexpr int kTargetGroups = 512;       // workgroups the weight-gradient grid aims for (two per CU)

template <typename T> struct FfnT;
template <> struct FfnT<__bf16> {
  typedef ff_bf16x8 vec;            // a 16-byte piece
  static constexpr int EPP = 8;     // elements of a 16-byte piece
  static constexpr int PAD = 8;     // LDS rows: + 16 bytes
};
template <> struct FfnT<float> {
  typedef ff_f32x4 vec;
  static constexpr int EPP = 4;
  static constexpr int PAD = 4;
};

// 8 k-values of one operand row (lane half h of a 16-wide k-step; eight 32x32x2 steps on fp32 rows)
template <typename T> struct Frag;
template <> struct Frag<__bf16> { ff_bf16x8 v; };
template <> struct Frag<float> { float v[8]; };

__device__ __forceinline__ void ffn_mma(ff_f32x16 &acc, const Frag<__bf16> &a, const Frag<__bf16> &b) {
  acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a.v, b.v, acc, 0, 0, 0);
}
__device__ __forceinline__ void ffn_mma(ff_f32x16 &acc, const Frag<float> &a, const Frag<float> &b) {
#pragma unroll
  for (int j = 0; j < 8; ++j) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a.v[j], b.v[j], acc, 0, 0, 0);
}

// 8 consecutive elements at p (16-byte aligned)
__device__ __forceinline__ Frag<__bf16> ffn_load8(const __bf16 *p) {
  Frag<__bf16> f;
  f.v = *reinterpret_cast<const ff_bf16x8 *>(p);
  return f;
}
__device__ __forceinline__ Frag<float> ffn_load8(const float *p) {
  Frag<float> f;
  const ff_f32x4 a = *reinterpret_cast<const ff_f32x4 *>(p), b = *reinterpret_cast<const ff_f32x4 *>(p + 4);
#pragma unroll
  for (int j = 0; j < 4; ++j) { f.v[j] = a[j]; f.v[4 + j] = b[j]; }
  return f;
}
// elements 0..3 at p, 4..7 at p + 8: the k order of an accumulator used as an operand
__device__ __forceinline__ Frag<__bf16> ffn_load44(const __bf16 *p) {
  Frag<__bf16> f;
  const ff_bf16x4 a = *reinterpret_cast<const ff_bf16x4 *>(p), b = *reinterpret_cast<const ff_bf16x4 *>(p + 8);
#pragma unroll
  for (int j = 0; j < 4; ++j) { f.v[j] = a[j]; f.v[4 + j] = b[j]; }
  return f;
}
__device__ __forceinline__ Frag<float> ffn_load44(const float *p) {
  Frag<float> f;
  const ff_f32x4 a = *reinterpret_cast<const ff_f32x4 *>(p), b = *reinterpret_cast<const ff_f32x4 *>(p + 8);
#pragma unroll
  for (int j = 0; j < 4; ++j) { f.v[j] = a[j]; f.v[4 + j] = b[j]; }
  return f;
}
// registers 8 s .. 8 s + 7 of a 32x32 tile as the fragment of k-step s (the one rounding of the hidden activation)
template <typename T> __device__ __forceinline__ Frag<T> ffn_acc_frag(const float (&x)[16], int s) {
  Frag<T> f;
#pragma unroll
  for (int j = 0; j < 8; ++j) f.v[j] = (T)x[8 * s + j];
  return f;
}
template <typename T> __device__ __forceinline__ Frag<T> ffn_zero_frag() {
  Frag<T> f;
#pragma unroll
  for (int j = 0; j < 8; ++j) f.v[j] = (T)0.f;
  return f;
}
// row of register reg of a 32x32 C/D tile in lane half h
__device__ __forceinline__ int ffn_row(int reg, int h) { return (reg & 3) + 8 * (reg >> 2) + 4 * h; }

__device__ __forceinline__ void ffn_zero(ff_f32x16 &a) {
#pragma unroll
  for (int i = 0; i < 16; ++i) a[i] = 0.f;
}

// 4 consecutive channels of one row
__device__ __forceinline__ void ffn_store4(__bf16 *p, float a, float b, float c, float d) {
  ff_bf16x4 v;
  v[0] = (__bf16)a; v[1] = (__bf16)b; v[2] = (__bf16)c; v[3] = (__bf16)d;
  *reinterpret_cast<ff_bf16x4 *>(p) = v;
}
__device__ __forceinline__ void ffn_store4(float *p, float a, float b, float c, float d) {
  ff_f32x4 v;
  v[0] = a; v[1] = b; v[2] = c; v[3] = d;
  *reinterpret_cast<ff_f32x4 *>(p) = v;
}

// ---- activations, in fp32 --------------------------------------------------------------------------------------------
template <int A> __device__ __forceinline__ float act_f(float v) {
  if constexpr (A == ME_FFN_RELU) return v > 0.f ? v : 0.f;
  else if constexpr (A == ME_FFN_GELU) return 0.5f * v * (1.f + erff(v * 0.70710678118654752f));
  else if constexpr (A == ME_FFN_GELU_TANH) {
    const float u = 0.79788456080286536f * (v + 0.044715f * v * v * v);
    return 0.5f * v * (1.f + tanhf(u));
  } else return v / (1.f + expf(-v));
}
template <int A> __device__ __forceinline__ float act_g(float v) {
  if constexpr (A == ME_FFN_RELU) return v > 0.f ? 1.f : 0.f;   // act'(0) = 0, as in torch
  else if constexpr (A == ME_FFN_GELU)
    return 0.5f * (1.f + erff(v * 0.70710678118654752f)) + v * 0.39894228040143268f * expf(-0.5f * v * v);
  else if constexpr (A == ME_FFN_GELU_TANH) {
    const float t = tanhf(0.79788456080286536f * (v + 0.044715f * v * v * v));
    return 0.5f * (1.f + t) + 0.5f * v * (1.f - t * t) * 0.79788456080286536f * (1.f + 3.f * 0.044715f * v * v);
  } else {
    const float s = 1.f / (1.f + expf(-v));
    return s * (1.f + v * (1.f - s));
  }
}

// rows x cols elements (cols a multiple of a piece) from src (row stride ld_src) into the LDS image dst (row stride ld_dst)
template <typename T>
__device__ __forceinline__ void stage(const T *__restrict__ src, int64_t ld_src, int rows, int cols, T *dst, int ld_dst) {
  constexpr int EPP = FfnT<T>::EPP;
  using vec = typename FfnT<T>::vec;
  const int ppr = cols / EPP;
  for (int p = threadIdx.x; p < rows * ppr; p += kThreads) {
    const int rr = p / ppr, pc = p - rr * ppr;
    *reinterpret_cast<vec *>(dst + rr * ld_dst + pc * EPP) =
        *reinterpret_cast<const vec *>(src + (int64_t)rr * ld_src + pc * EPP);
  }
}

// a wave's fragment of 8 channels of 32 rows into its transposed image [channel][row]
template <typename T> __device__ __forceinline__ void scatter_t(T *s_t, int ldt, int ch0, int r, const Frag<T> &f) {
#pragma unroll
  for (int j = 0; j < 8; ++j) s_t[(ch0 + j) * ldt + r] = f.v[j];
}

// ---- dst [cols, rows] = src [rows, cols]^T; both dimensions multiples of 32 ------------------------------------------
template <typename T>
__global__ __launch_bounds__(kThreads) void k_ffn_transpose(const T *__restrict__ src, T *__restrict__ dst, int rows,
                                                            int cols) {
  __shared__ T tile[32][33];
  const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
  const int r0 = blockIdx.y * 32, c0 = blockIdx.x * 32;
#pragma unroll
  for (int i = 0; i < 4; ++i) tile[ty + 8 * i][tx] = src[(int64_t)(r0 + ty + 8 * i) * cols + c0 + tx];
  __syncthreads();
#pragma unroll
  for (int i = 0; i < 4; ++i) dst[(int64_t)(c0 + ty + 8 * i) * rows + r0 + tx] = tile[tx][ty + 8 * i];
}

// ---- host side ----------------------------------------------------------------------------------------------------------
template <typename K> inline int allow_lds(K fn, int64_t lds) {
  if (lds > 48 * 1024)
    ME_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(fn), hipFuncAttributeMaxDynamicSharedMemorySize, kLdsBudget));
  return 0;
}

template <typename T> int transpose(const T *src, T *dst, int rows, int cols, hipStream_t stream) {
  hipLaunchKernelGGL(k_ffn_transpose<T>, dim3((unsigned)(cols / 32), (unsigned)(rows / 32)), dim3(kThreads), 0, stream,
                     src, dst, rows, cols);
  ME_LAUNCH_CHECK();
  return 0;
}

inline bool aligned16(std::initializer_list<const void *> ps) {
  for (const void *p : ps)
    if (((uintptr_t)p & 15) != 0) return false;
  return true;
}

}  // namespace ffn
}  // namespace me
