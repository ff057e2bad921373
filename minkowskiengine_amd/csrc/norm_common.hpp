// Shared by the normalisation translation units (norm.hip: batch norm over all rows, instance_norm.hip: the same
// arithmetic segmented by the batch index of each row): the chunking of the two-level reductions, the fixed-order LDS
// combine of the row lanes, the launch plan (SegPlan) and the dispatch over the piece width and the row type.  Rows are
// read as pieces widened to fp32 (piece.hpp), their width chosen by kPieceNorm.
#pragma once
#include "piece.hpp"

namespace me {

constexpr int kBnMaxChunks = 512;
constexpr int kBnRowsPerThread = 8;   // fully unrolled: 8 rows in flight per thread (2 or 4 with more workgroups
                                      // measured 2x slower: the loads in flight per thread matter, not the grid size)

// max(v, 0) that keeps a NaN (fmaxf returns the other operand): a non-finite row must reach M2 and rstd, as it does in
// torch and in the float64 twins of the instance norm, not come out as a variance of 0
__device__ __forceinline__ float clamp_neg(float v) { return v < 0.f ? 0.f : v; }
// the fused ReLU of the apply kernels: fmaxf(v, 0) for every number (the same bits), NaN for a NaN as torch's relu
__device__ __forceinline__ float relu_keep_nan(float v) { return v != v ? v : fmaxf(v, 0.f); }

// LDS of the partial kernels: s_red[R][2c] (one row of 2c sums per row lane) | s_out[2c] | s_tmp[256] | s_shift[c]
// (s_tmp is bn_reduce_lanes' scratch; between two calls of it the instance-norm partial kernels keep the 4 ints of their
// chunk scans in s_tmp[0..3], so bn_reduce_lanes must not touch s_tmp before its leading barrier or after its trailing one)
__host__ __device__ constexpr size_t bn_partial_lds_bytes(int c, int row_lanes) {
  return ((size_t)row_lanes * 2 * c + 2 * c + 256 + c) * sizeof(float);
}

// s_out[q] = sum over the row lanes l (ascending) of s_red[l * 2c + q], by the whole workgroup: with fewer than 256
// values (c < 128) G = 256 / 2c threads share a value — contiguous lane ranges, their G partial sums added in range
// order — instead of c / V threads walking all R lanes (R = 32 - 64 on the narrow layers: 500 - 1000 serial LDS reads
// on a handful of threads were 5 - 10 us of every partial kernel).  A fixed order: bitwise reproducible.
__device__ __forceinline__ void bn_reduce_lanes(const float *__restrict__ s_red, float *__restrict__ s_out,
                                                float *__restrict__ s_tmp, int c, int R) {
  const int NV = 2 * c, tid = (int)threadIdx.x, NT = (int)blockDim.x;
  __syncthreads();
  if (NV * 2 > NT) {
    for (int q = tid; q < NV; q += NT) {
      float a = 0.f;
      for (int l = 0; l < R; ++l) a += s_red[l * NV + q];
      s_out[q] = a;
    }
  } else {
    const int G = NT / NV, g = tid / NV, q = tid % NV;
    if (g < G) {
      float a = 0.f;
      for (int l = g * R / G; l < (g + 1) * R / G; ++l) a += s_red[l * NV + q];
      s_tmp[g * NV + q] = a;
    }
    __syncthreads();
    if (tid < NV) {
      float a = 0.f;
      for (int gg = 0; gg < G; ++gg) a += s_tmp[gg * NV + tid];
      s_out[tid] = a;
    }
  }
  __syncthreads();
}

// per-channel parameters of V consecutive channels (gamma / beta may be NULL: 1 / 0 — one uniform branch, not one
// per element)
template <int V>
__device__ __forceinline__ void load_affine(const float *__restrict__ gamma, const float *__restrict__ beta, int ch0,
                                            float (&ga)[V], float (&be)[V]) {
  if (gamma != nullptr) {
#pragma unroll
    for (int j = 0; j < V; ++j) ga[j] = gamma[ch0 + j];
  } else {
#pragma unroll
    for (int j = 0; j < V; ++j) ga[j] = 1.f;
  }
  if (beta != nullptr) {
#pragma unroll
    for (int j = 0; j < V; ++j) be[j] = beta[ch0 + j];
  } else {
#pragma unroll
    for (int j = 0; j < V; ++j) be[j] = 0.f;
  }
}

// chunks of a reduction over n rows by workgroups of `row_lanes` row lanes: one batch of rows in flight per thread
// where that fills the chip (rows_per_thread * row_lanes rows per chunk), more per thread beyond kBnMaxChunks chunks
static int bn_chunks(int64_t n, int row_lanes, int rows_per_thread) {
  int64_t g = ceil_div(n, (int64_t)row_lanes * rows_per_thread);
  if (g > kBnMaxChunks) g = kBnMaxChunks;
  if (g < 1) g = 1;
  return (int)g;
}
static int bn_chunks_max(int64_t n) { return bn_chunks(n, 1, kBnRowsPerThread / 2); }   // workspace bound

// The launch of the kernels over rows of c channels of T: v channels per piece (kPieceNorm of the pointers whose
// alignment counts), P pieces per row, R row lanes per workgroup; `chunks` workgroups of `lds` bytes for a partial kernel
// with `rows_in_flight` rows per thread, `grid` workgroups for a row kernel (k_bn_apply, seg_rows)
struct SegPlan {
  int v, P, R, chunks;
  size_t lds;
  dim3 grid;
};
template <typename T>
static SegPlan seg_plan(int64_t n, int c, int rows_in_flight, std::initializer_list<const void *> ptrs) {
  SegPlan pl;
  pl.v = piece_width<T>(kPieceNorm, c, ptrs);
  pl.P = c / pl.v;
  pl.R = pl.P >= 256 ? 1 : 256 / pl.P;
  pl.chunks = bn_chunks(n, pl.R, rows_in_flight);
  pl.lds = bn_partial_lds_bytes(c, pl.R);
  pl.grid = dim3((unsigned)ceil_div(n, (int64_t)pl.R * kBnRowsPerThread));
  return pl;
}

// the body of an extern "C" entry point whose rows are float or, with is_bf16, __bf16: `return call;` with T the row type
#define ME_SEG_RETURN_T(is_bf16, ...)          \
  do {                                         \
    if (is_bf16) {                             \
      using T = __bf16;                        \
      return __VA_ARGS__;                      \
    }                                          \
    using T = float;                           \
    return __VA_ARGS__;                        \
  } while (0)

}  // namespace me
