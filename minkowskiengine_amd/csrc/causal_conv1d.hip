// Causal depthwise conv1d (+ SiLU) along the serialized voxel order, for gfx950 (MI355X): MinkowskiFunctional.causal_conv1d
// and the local mixing of MinkowskiMamba (ABI 1.28).  The sequence is the selective scan's: position p is row seg_rows[p]
// (seg_rows[n - 1 - p] with `reverse`), every instance along its curve, instance after instance; a position whose row has
// another batch_row than the position before it starts an instance.  With K taps, weight [D, K] and bias [D] in fp32:
//   pre[row_p, d] = bias[d] + sum_{j < K} weight[d, K - 1 - j] x[row_{p - j}, d]      tap j only where j positions of the
//   y = pre, or silu(pre)                                                             same instance precede p
// Everything is fp32 in registers; bf16 rows are rounded once at the store.  A depthwise operator has one multiply-add a
// loaded element and tap: nothing to put on the matrix pipe, the kernels are bound by their row traffic.
//
// Work split.  The grid is (runs of consecutive chunks, channel slabs); a chunk is kChunk = 256 positions.  The 256 threads
// of a workgroup are L channel lanes x (256 / L) position teams.  A lane owns V consecutive channels: one 16-byte access
// (4 fp32, 8 bf16) where D, the base pointers and the row strides allow it, else V = 1.  The ceil(D / V) pieces are spread
// evenly over ceil(pieces / 64) slabs, so L <= 64 is whatever the slab needs (64 at D = 256 fp32, 1 at D = 1) and the teams
// fill the rest of the workgroup: a team walks a contiguous piece of ceil(256 / teams) positions of the chunk.
//
// LDS.  Once per chunk the workgroup stages the rows of the chunk's positions with a halo of K - 1 on both sides (-1 past
// either end of the sequence), and for every position "how many positions of the same instance precede it, clamped to
// K - 1", from batch_row of at most K - 1 earlier positions.  The step loops read both and do no index arithmetic.
//
// Forward.  A team preloads the K - 1 rows before its piece and slides a window of K values a channel: every row of x is
// read once a walk, plus the halo.  The rows of the next kAhead positions are loaded while those of the current ones are
// used.  weight and bias of the lane's channels stay in registers over the run of chunks.
//
// Backward recomputes pre from x (nothing but the operands is saved; without SiLU there is nothing to recompute).  A team
// reads x and dy of its piece and of K - 1 positions after it, forms g = dy act'(pre) there and slides a window of K
// values of g:  dx[row_p] = sum_j weight[d, K - 1 - j] g[p + j]  under the mask of position p + j.  dweight (K values a
// channel) and dbias are summed in registers over the team's OWN positions across the whole run of chunks; at the end the
// teams are added through LDS in ascending order and the workgroup writes one record [K + 1][slab channels] into
// [runs][K + 1][D]; k_cconv_reduce adds the runs in ascending order.  Both merges carry the rounding error of every
// addition along (add_compensated): at D = 1 the 256 teams own one position each, and a plain ascending sum of that
// length lost a digit against torch's blocked sum.  No atomics: every output is bitwise reproducible.
#include "common.hpp"
#include "piece.hpp"

namespace me {
namespace cconv {

constexpr int kChunk = 256;         // positions a chunk (me_cconv_chunk)
constexpr int kThreads = 256;
constexpr int kMaxLanes = 64;       // channel lanes of a workgroup at most: a slab is up to 64 V channels
constexpr int kMaxRuns = ME_CCONV_MAX_RUNS;
constexpr int kAhead = 4;           // positions whose rows are in flight before they are used

struct Args {
  const void *x, *dy;               // dy: backward only
  int64_t x_stride, dy_stride;
  const float *weight, *bias;
  const int32_t *seg_rows, *batch_row;
  int64_t n;
  int32_t d, reverse;
  int32_t lanes, teams, piece;      // the split of a workgroup
  int32_t nchunks, run_chunks;
  void *out;                        // y (forward) or dx (backward, may be NULL)
  int64_t out_stride;
  float *part;                      // backward: [runs][K + 1][d], NULL when neither dweight nor dbias is wanted
};

__device__ __forceinline__ float sigmoid_f(float x) { return 1.f / (1.f + expf(-x)); }

// sum += v with the rounding error of the addition carried in `lost` (Kahan): the merges of up to 256 teams and of up to
// kMaxRuns records stay ascending sums, but do not lose a digit to their length
__device__ __forceinline__ void add_compensated(float &sum, float &lost, float v) {
  const float y = v - lost, t = sum + y;
  lost = (t - sum) - y;
  sum = t;
}

// rows of the positions c0 - (K - 1) .. c0 + kChunk + K - 2 (-1 outside the sequence) and, for the positions
// c0 .. c0 + kChunk + K - 2, the number of same-instance predecessors clamped to K - 1
template <int K>
__device__ __forceinline__ void stage_chunk(const Args &a, int64_t c0, int32_t *rowv, int32_t *batv, int32_t *cnt) {
  constexpr int H = K - 1;
  for (int i = threadIdx.x; i < kChunk + 2 * H; i += kThreads) {
    const int64_t p = c0 - H + i;
    int32_t row = -1, bat = -1;
    if (p >= 0 && p < a.n) {
      row = a.seg_rows[a.reverse ? a.n - 1 - p : p];
      bat = a.batch_row[row];
    }
    rowv[i] = row;
    batv[i] = bat;
  }
  __syncthreads();
  for (int t = threadIdx.x; t < kChunk + H; t += kThreads) {
    int c = 0;
    if (rowv[t + H] >= 0) {
      const int32_t mine = batv[t + H];
#pragma unroll
      for (int j = 1; j <= H; ++j)
        if (c == j - 1 && rowv[t + H - j] >= 0 && batv[t + H - j] == mine) c = j;
    }
    cnt[t] = c;
  }
  __syncthreads();
}

template <typename T, int K, int V, bool SILU>
__global__ __launch_bounds__(kThreads) void k_cconv_fwd(Args a) {
  constexpr int H = K - 1;
  __shared__ int32_t rowv[kChunk + 2 * H], batv[kChunk + 2 * H], cnt[kChunk + H];
  const int tid = threadIdx.x, team = tid / a.lanes, lane = tid - team * a.lanes;
  const int ch = ((int)blockIdx.y * a.lanes + lane) * V;
  const bool on = team < a.teams && ch < a.d;
  const T *x = (const T *)a.x + ch;
  T *y = (T *)a.out + ch;
  float w[K][V], b[V];
#pragma unroll
  for (int v = 0; v < V; ++v) {
#pragma unroll
    for (int k = 0; k < K; ++k) w[k][v] = on ? a.weight[(int64_t)(ch + v) * K + k] : 0.f;
    b[v] = (on && a.bias != nullptr) ? a.bias[ch + v] : 0.f;
  }
  const int64_t first = (int64_t)blockIdx.x * a.run_chunks;
  const int64_t last = first + a.run_chunks < a.nchunks ? first + a.run_chunks : a.nchunks;
  for (int64_t chunk = first; chunk < last; ++chunk) {
    const int64_t c0 = chunk * kChunk;
    const int nt = (int)(a.n - c0 < kChunk ? a.n - c0 : kChunk);
    __syncthreads();                          // the chunk before has been read out of LDS
    stage_chunk<K>(a, c0, rowv, batv, cnt);
    const int s0 = team * a.piece, s1 = s0 + a.piece < nt ? s0 + a.piece : nt;
    if (!on || s0 >= s1) continue;
    Piece<V> back[K];                         // back[j]: x of the position j before the current one (j >= 1)
#pragma unroll
    for (int j = 1; j <= H; ++j) {
      const int32_t row = rowv[s0 + H - j];
#pragma unroll
      for (int v = 0; v < V; ++v) back[j].v[v] = 0.f;
      if (row >= 0) back[j] = load_piece<T, V>(x + (int64_t)row * a.x_stride);
    }
    Piece<V> cur[kAhead], nxt[kAhead];
#pragma unroll
    for (int u = 0; u < kAhead; ++u)
      if (s0 + u < s1) cur[u] = load_piece<T, V>(x + (int64_t)rowv[s0 + u + H] * a.x_stride);
    for (int t0 = s0; t0 < s1; t0 += kAhead) {
#pragma unroll
      for (int u = 0; u < kAhead; ++u)
        if (t0 + kAhead + u < s1) nxt[u] = load_piece<T, V>(x + (int64_t)rowv[t0 + kAhead + u + H] * a.x_stride);
#pragma unroll
      for (int u = 0; u < kAhead; ++u) {
        const int t = t0 + u;
        if (t < s1) {
          const int c = cnt[t];
          Piece<V> r;
#pragma unroll
          for (int v = 0; v < V; ++v) {
            float acc = b[v];
#pragma unroll
            for (int j = H; j >= 1; --j)
              if (c >= j) acc = fmaf(w[H - j][v], back[j].v[v], acc);
            acc = fmaf(w[H][v], cur[u].v[v], acc);
            r.v[v] = SILU ? acc * sigmoid_f(acc) : acc;
          }
          store_piece<T, V>(y + (int64_t)rowv[t + H] * a.out_stride, r);
#pragma unroll
          for (int j = H; j >= 2; --j) back[j] = back[j - 1];
          back[1] = cur[u];
        }
      }
#pragma unroll
      for (int u = 0; u < kAhead; ++u) cur[u] = nxt[u];
    }
  }
}

template <typename T, int K, int V, bool SILU>
__global__ __launch_bounds__(kThreads) void k_cconv_bwd(Args a) {
  constexpr int H = K - 1;
  __shared__ int32_t rowv[kChunk + 2 * H], batv[kChunk + 2 * H], cnt[kChunk + H];
  __shared__ float red[kThreads * V];
  const int tid = threadIdx.x, team = tid / a.lanes, lane = tid - team * a.lanes;
  const int ch = ((int)blockIdx.y * a.lanes + lane) * V;
  const bool on = team < a.teams && ch < a.d;
  const T *x = (const T *)a.x + ch, *dy = (const T *)a.dy + ch;
  T *dx = a.out == nullptr ? nullptr : (T *)a.out + ch;
  float w[K][V], b[V], dw[K + 1][V];          // dw[K]: dbias
#pragma unroll
  for (int v = 0; v < V; ++v) {
#pragma unroll
    for (int k = 0; k < K; ++k) {
      w[k][v] = on ? a.weight[(int64_t)(ch + v) * K + k] : 0.f;
      dw[k][v] = 0.f;
    }
    dw[K][v] = 0.f;
    b[v] = (on && a.bias != nullptr) ? a.bias[ch + v] : 0.f;
  }
  const int64_t first = (int64_t)blockIdx.x * a.run_chunks;
  const int64_t last = first + a.run_chunks < a.nchunks ? first + a.run_chunks : a.nchunks;
  for (int64_t chunk = first; chunk < last; ++chunk) {
    const int64_t c0 = chunk * kChunk;
    const int nt = (int)(a.n - c0 < kChunk ? a.n - c0 : kChunk);
    __syncthreads();                          // the chunk before has been read out of LDS
    stage_chunk<K>(a, c0, rowv, batv, cnt);
    const int s0 = team * a.piece, s1 = s0 + a.piece < nt ? s0 + a.piece : nt;
    if (!on || s0 >= s1) continue;
    Piece<V> back[K];                         // back[j]: x of the position j before the current one (j >= 1)
#pragma unroll
    for (int j = 1; j <= H; ++j) {
      const int32_t row = rowv[s0 + H - j];
#pragma unroll
      for (int v = 0; v < V; ++v) back[j].v[v] = 0.f;
      if (row >= 0) back[j] = load_piece<T, V>(x + (int64_t)row * a.x_stride);
    }
    Piece<V> gw[K];                           // gw[j]: g of the position j before the current one; cw: its count
    int cw[K];
#pragma unroll
    for (int j = 0; j < K; ++j) {
      cw[j] = 0;
#pragma unroll
      for (int v = 0; v < V; ++v) gw[j].v[v] = 0.f;
    }
    // the positions s0 .. s1 + H - 1: the team's own and the H after them, which complete dx of the last own ones
    for (int t0 = s0; t0 < s1 + H; t0 += kAhead) {
      Piece<V> xv[kAhead], gv[kAhead];
#pragma unroll
      for (int u = 0; u < kAhead; ++u) {
#pragma unroll
        for (int v = 0; v < V; ++v) xv[u].v[v] = gv[u].v[v] = 0.f;
        if (t0 + u < s1 + H) {
          const int32_t row = rowv[t0 + u + H];
          if (row >= 0) {
            xv[u] = load_piece<T, V>(x + (int64_t)row * a.x_stride);
            gv[u] = load_piece<T, V>(dy + (int64_t)row * a.dy_stride);
          }
        }
      }
#pragma unroll
      for (int u = 0; u < kAhead; ++u) {
        const int i = t0 + u;
        if (i < s1 + H) {
          const int c = rowv[i + H] >= 0 ? cnt[i] : 0;
          const bool own = i < s1;
#pragma unroll
          for (int j = H; j >= 1; --j) {
            gw[j] = gw[j - 1];
            cw[j] = cw[j - 1];
          }
          cw[0] = c;
#pragma unroll
          for (int v = 0; v < V; ++v) {
            float g = gv[u].v[v];
            if (SILU) {
              float pre = b[v];
#pragma unroll
              for (int j = H; j >= 1; --j)
                if (c >= j) pre = fmaf(w[H - j][v], back[j].v[v], pre);
              pre = fmaf(w[H][v], xv[u].v[v], pre);
              const float s = sigmoid_f(pre);
              g *= s * (1.f + pre * (1.f - s));
            }
            gw[0].v[v] = g;
            if (own) {
              dw[K][v] += g;
              dw[H][v] = fmaf(g, xv[u].v[v], dw[H][v]);
#pragma unroll
              for (int j = 1; j <= H; ++j)
                if (c >= j) dw[H - j][v] = fmaf(g, back[j].v[v], dw[H - j][v]);
            }
          }
          const int p = i - H;                // gw[H - j] is g of position p + j
          if (p >= s0 && dx != nullptr) {
            Piece<V> r;
#pragma unroll
            for (int v = 0; v < V; ++v) {
              float acc = 0.f;
#pragma unroll
              for (int j = 0; j <= H; ++j)
                if (cw[H - j] >= j) acc = fmaf(w[H - j][v], gw[H - j].v[v], acc);
              r.v[v] = acc;
            }
            store_piece<T, V>(dx + (int64_t)rowv[p + H] * a.out_stride, r);
          }
#pragma unroll
          for (int j = H; j >= 2; --j) back[j] = back[j - 1];
          back[1] = xv[u];
        }
      }
    }
  }
  if (a.part == nullptr) return;
  // the teams in ascending order, one of the K + 1 values a channel at a time
  const int slab_ch = a.lanes * V, ch0 = (int)blockIdx.y * slab_ch;
  float *rec = a.part + (int64_t)blockIdx.x * (K + 1) * a.d;
#pragma unroll
  for (int k = 0; k <= K; ++k) {
    __syncthreads();
#pragma unroll
    for (int v = 0; v < V; ++v) red[tid * V + v] = dw[k][v];
    __syncthreads();
    for (int c = tid; c < slab_ch; c += kThreads) {
      if (ch0 + c >= a.d) continue;
      float r = red[c], lost = 0.f;
      for (int t = 1; t < a.teams; ++t) add_compensated(r, lost, red[t * slab_ch + c]);
      rec[(int64_t)k * a.d + ch0 + c] = r;
    }
  }
}

// dweight [d, K] and dbias [d] = the runs' records [K + 1][d], added in ascending run order (no records: zeros)
__global__ __launch_bounds__(256) void k_cconv_reduce(const float *__restrict__ part, int nruns, int d, int K,
                                                      float *__restrict__ dweight, float *__restrict__ dbias) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int64_t rec = (int64_t)d * (K + 1);
  if (i >= rec) return;
  float r = 0.f, lost = 0.f;
#pragma unroll 8
  for (int run = 0; run < nruns; ++run) add_compensated(r, lost, part[run * rec + i]);
  const int k = (int)(i / d), c = (int)(i % d);
  if (k < K) {
    if (dweight != nullptr) dweight[(int64_t)c * K + k] = r;
  } else if (dbias != nullptr) {
    dbias[c] = r;
  }
}

// ---- launch policy (host) -------------------------------------------------------------------------------------------
inline int64_t chunks_of(int64_t n) { return ceil_div(n, kChunk); }
inline int run_chunks_of(int64_t nchunks) { return (int)ceil_div(nchunks, kMaxRuns); }
inline int64_t runs_of(int64_t n) {
  const int64_t nch = chunks_of(n);
  return nch == 0 ? 0 : ceil_div(nch, run_chunks_of(nch));
}

// the split of a workgroup for d channels in pieces of v: slabs, lanes, teams, positions a team
struct Split {
  int slabs, lanes, teams, piece;
};
inline Split split_of(int d, int v) {
  const int pieces = d / v;
  Split s;
  s.slabs = (int)ceil_div(pieces, kMaxLanes);
  s.lanes = (int)ceil_div(pieces, s.slabs);
  s.teams = kThreads / s.lanes;
  s.piece = (int)ceil_div(kChunk, s.teams);
  return s;
}

// 16-byte pieces where the channel count, the base pointers and the row strides allow them
template <typename T>
inline int width_of(int d, std::initializer_list<const void *> ptrs, std::initializer_list<int64_t> strides) {
  constexpr int W = 16 / (int)sizeof(T);
  if (d % W != 0 || !aligned(ptrs, 16)) return 1;
  for (int64_t s : strides)
    if (s % W != 0) return 1;
  return W;
}

template <typename T, int K, bool BWD>
int launch(Args a, int v, bool silu, hipStream_t stream) {
  const Split s = split_of(a.d, v);
  a.lanes = s.lanes, a.teams = s.teams, a.piece = s.piece;
  a.nchunks = (int32_t)chunks_of(a.n);
  a.run_chunks = run_chunks_of(a.nchunks);
  const dim3 grid((unsigned)runs_of(a.n), (unsigned)s.slabs);
  constexpr int W = 16 / (int)sizeof(T);
#define ME_CCONV_GO(V, S)                                                                              \
  do {                                                                                                 \
    if (BWD) hipLaunchKernelGGL((k_cconv_bwd<T, K, V, S>), grid, dim3(kThreads), 0, stream, a);        \
    else hipLaunchKernelGGL((k_cconv_fwd<T, K, V, S>), grid, dim3(kThreads), 0, stream, a);            \
  } while (0)
  if (v == W) {
    if (silu) ME_CCONV_GO(W, true);
    else ME_CCONV_GO(W, false);
  } else {
    if (silu) ME_CCONV_GO(1, true);
    else ME_CCONV_GO(1, false);
  }
#undef ME_CCONV_GO
  ME_LAUNCH_CHECK();
  return 0;
}

template <typename T, bool BWD>
int launch_k(const Args &a, int k, int v, bool silu, hipStream_t stream) {
  return k == 2 ? launch<T, 2, BWD>(a, v, silu, stream)
                : k == 3 ? launch<T, 3, BWD>(a, v, silu, stream) : launch<T, 4, BWD>(a, v, silu, stream);
}

}  // namespace cconv
}  // namespace me

using namespace me;

#define ME_CCONV_CHECK_SHAPE(n, d, k)                                                                \
  ME_CHECK(me_cconv_supported(d, k, 0) != 0, "the kernels serve d >= 1 channels and k = 2, 3 or 4 taps"); \
  ME_CHECK(n >= 0 && n < ((int64_t)1 << 31), "n must be in [0, 2^31)")

extern "C" {

int32_t me_cconv_supported(int32_t d, int32_t k, int32_t is_bf16) {
  (void)is_bf16;
  return (d >= 1 && k >= 2 && k <= 4) ? 1 : 0;
}

int32_t me_cconv_chunk(void) { return cconv::kChunk; }

int64_t me_cconv_workspace_bytes(int64_t n, int32_t d, int32_t k, int32_t backward) {
  if (n <= 0 || d < 1 || k < 1 || backward == 0) return 0;
  return cconv::runs_of(n) * (k + 1) * (int64_t)d * (int64_t)sizeof(float);
}

int me_cconv_forward(const void *x_dev, int32_t is_bf16, int64_t x_stride, const float *weight_dev, const float *bias_dev,
                     int32_t silu, const int32_t *seg_rows_dev, const int32_t *batch_row_dev, int32_t reverse, int64_t n,
                     int32_t d, int32_t k, void *y_dev, int64_t y_stride, void *stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  ME_CCONV_CHECK_SHAPE(n, d, k);
  ME_CHECK(x_stride >= d && y_stride >= d, "a row stride must be at least d");
  if (n == 0) return 0;
  ME_CHECK(x_dev != nullptr && weight_dev != nullptr && y_dev != nullptr, "x, weight and y must be given");
  ME_CHECK(seg_rows_dev != nullptr && batch_row_dev != nullptr, "the sequence rows and the instance of every row must be given");
  const int elem = is_bf16 ? 2 : 4;
  ME_CHECK(aligned({x_dev, y_dev}, elem) && aligned({weight_dev, bias_dev, seg_rows_dev, batch_row_dev}, 4),
           "the operands must be aligned to their element");
  cconv::Args a{};
  a.x = x_dev, a.x_stride = x_stride, a.weight = weight_dev, a.bias = bias_dev;
  a.seg_rows = seg_rows_dev, a.batch_row = batch_row_dev, a.n = n, a.d = d, a.reverse = reverse ? 1 : 0;
  a.out = y_dev, a.out_stride = y_stride;
  if (is_bf16)
    return cconv::launch_k<__bf16, false>(a, k, cconv::width_of<__bf16>(d, {x_dev, y_dev}, {x_stride, y_stride}), silu != 0,
                                          stream);
  return cconv::launch_k<float, false>(a, k, cconv::width_of<float>(d, {x_dev, y_dev}, {x_stride, y_stride}), silu != 0,
                                       stream);
}

int me_cconv_backward(const void *x_dev, const void *dy_dev, int32_t is_bf16, int64_t x_stride, int64_t dy_stride,
                      const float *weight_dev, const float *bias_dev, int32_t silu, const int32_t *seg_rows_dev,
                      const int32_t *batch_row_dev, int32_t reverse, int64_t n, int32_t d, int32_t k, void *dx_dev,
                      int64_t dx_stride, float *dweight_dev, float *dbias_dev, void *workspace_dev, int64_t workspace_bytes,
                      void *stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  ME_CCONV_CHECK_SHAPE(n, d, k);
  ME_CHECK(x_stride >= d && dy_stride >= d && (dx_dev == nullptr || dx_stride >= d), "a row stride must be at least d");
  ME_CHECK(dbias_dev == nullptr || bias_dev != nullptr, "the gradient of bias needs bias");
  const bool sums = dweight_dev != nullptr || dbias_dev != nullptr;
  const unsigned reduce_blocks = (unsigned)ceil_div((int64_t)d * (k + 1), 256);
  if (n == 0) {                                       // no rows: the parameter gradients are sums of no records
    if (sums) {
      hipLaunchKernelGGL(cconv::k_cconv_reduce, dim3(reduce_blocks), dim3(256), 0, stream, (const float *)nullptr, 0, d, k,
                         dweight_dev, dbias_dev);
      ME_LAUNCH_CHECK();
    }
    return 0;
  }
  ME_CHECK(x_dev != nullptr && dy_dev != nullptr && weight_dev != nullptr, "x, dy and weight must be given");
  ME_CHECK(seg_rows_dev != nullptr && batch_row_dev != nullptr, "the sequence rows and the instance of every row must be given");
  ME_CHECK(workspace_dev != nullptr && workspace_bytes >= me_cconv_workspace_bytes(n, d, k, 1),
           "the workspace is smaller than me_cconv_workspace_bytes");
  const int elem = is_bf16 ? 2 : 4;
  ME_CHECK(aligned({x_dev, dy_dev, dx_dev}, elem) &&
               aligned({weight_dev, bias_dev, seg_rows_dev, batch_row_dev, dweight_dev, dbias_dev, workspace_dev}, 4),
           "the operands must be aligned to their element");
  cconv::Args a{};
  a.x = x_dev, a.dy = dy_dev, a.x_stride = x_stride, a.dy_stride = dy_stride, a.weight = weight_dev, a.bias = bias_dev;
  a.seg_rows = seg_rows_dev, a.batch_row = batch_row_dev, a.n = n, a.d = d, a.reverse = reverse ? 1 : 0;
  a.out = dx_dev, a.out_stride = dx_dev == nullptr ? d : dx_stride;
  a.part = sums ? (float *)workspace_dev : nullptr;
  const std::initializer_list<const void *> ptrs = {x_dev, dy_dev, dx_dev};
  const std::initializer_list<int64_t> strides = {x_stride, dy_stride, a.out_stride};
  const int rc = is_bf16 ? cconv::launch_k<__bf16, true>(a, k, cconv::width_of<__bf16>(d, ptrs, strides), silu != 0, stream)
                         : cconv::launch_k<float, true>(a, k, cconv::width_of<float>(d, ptrs, strides), silu != 0, stream);
  if (rc != 0) return rc;
  if (sums) {
    hipLaunchKernelGGL(cconv::k_cconv_reduce, dim3(reduce_blocks), dim3(256), 0, stream, (const float *)workspace_dev,
                       (int)cconv::runs_of(n), d, k, dweight_dev, dbias_dev);
    ME_LAUNCH_CHECK();
  }
  return 0;
}

}  // extern "C"
