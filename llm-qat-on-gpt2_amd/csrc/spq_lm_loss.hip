// The language-model loss of SPLMHeadModel.forward (models_sp.py:443-449: shift, then F.cross_entropy) as row kernels, fp32
// (DESIGN.md 3.15).  Forward: one online max / sum pass over each logit row where it lies -> the row's log-sum-exp and the
// label's negative log-likelihood; a second, single-workgroup launch sums the rows in a fixed order.  Backward: softmax - onehot
// written straight into the full-size gradient, the probabilities recomputed from the saved log-sum-exp.
//
// One plan for every V: a 256-thread workgroup per row; thread t owns the 16-byte chunks t, t + 256, t + 512, ... of the row,
// counted from the ROW's first element, and thread 0 the V % 4 elements behind the last chunk.  A chunk is one dwordx4 load at
// 4-byte alignment (what gfx950 global loads and stores need, and what the compiler emits for a 16-byte copy through a float
// pointer), so V = 50257 and a base that is only 4-byte aligned need no peeled head: the cut of a row into chunks, and with it every
// rounding, is the same at all four phases of a 16-byte line.
#include <math.h>

#include "spq_common.h"

namespace spq {
namespace {

constexpr int LM_THREADS = 256;          // per row
constexpr int LM_UNROLL = 4;             // chunks a thread loads before it consumes one
constexpr int LM_REDUCE_THREADS = 1024;  // the single workgroup of the row sum
constexpr int64_t LM_MAX_GRID = 1 << 20; // rows beyond it are taken by a stride over the grid

// a 16-byte chunk at 4-byte alignment
__device__ __forceinline__ float4 load4(const float* p) {
  float4 v;
  __builtin_memcpy(&v, p, sizeof(v));
  return v;
}
__device__ __forceinline__ void store4(float* p, const float4& v) { __builtin_memcpy(p, &v, sizeof(v)); }

// running maximum m and sum s of exp(x - m).  -inf entries are allowed (probability 0): while the maximum is still -inf the
// exponent's offset is 0, so exp(-inf - 0) = 0 instead of exp(-inf + inf) = NaN.  fmaxf drops a NaN entry, the sum keeps it.
struct MaxSum {
  float m, s;
};
__device__ __forceinline__ float finite_offset(float m) { return m == -INFINITY ? 0.f : m; }
__device__ __forceinline__ void ms_add(MaxSum& a, float x) {
  const float mn = fmaxf(a.m, x), o = finite_offset(mn);
  a.s = a.s * __expf(a.m - o) + __expf(x - o);
  a.m = mn;
}
__device__ __forceinline__ void ms_add4(MaxSum& a, const float4& v) {
  const float mn = fmaxf(a.m, fmaxf(fmaxf(v.x, v.y), fmaxf(v.z, v.w))), o = finite_offset(mn);
  a.s = a.s * __expf(a.m - o) + ((__expf(v.x - o) + __expf(v.y - o)) + (__expf(v.z - o) + __expf(v.w - o)));
  a.m = mn;
}
// symmetric in its arguments, bit for bit: both lanes of a butterfly step get the same pair
__device__ __forceinline__ MaxSum ms_merge(const MaxSum& a, const MaxSum& b) {
  const float mn = fmaxf(a.m, b.m), o = finite_offset(mn);
  return MaxSum{mn, a.s * __expf(a.m - o) + b.s * __expf(b.m - o)};
}

// the label row (b, t) is scored against, or `ignore` when it has none
__device__ __forceinline__ int64_t row_label(const int64_t* __restrict__ labels, int64_t row, int T, int shift, int64_t ignore) {
  return ((int)(row % T) + shift < T) ? labels[row + shift] : ignore;
}

__global__ __launch_bounds__(LM_THREADS) void lm_cross_entropy_fwd_kernel(const float* __restrict__ logits,
                                                                          const int64_t* __restrict__ labels, int64_t rows, int T,
                                                                          int V, int shift, int64_t ignore,
                                                                          float* __restrict__ nll, float* __restrict__ lse) {
  __shared__ float wave_m[LM_THREADS / 64], wave_s[LM_THREADS / 64];
  const int tid = threadIdx.x, nvec = V >> 2;
  for (int64_t row = blockIdx.x; row < rows; row += gridDim.x) {
    const float* x = logits + row * V;
    MaxSum a{-INFINITY, 0.f};
    for (int c0 = tid; c0 < nvec; c0 += LM_THREADS * LM_UNROLL) {
      float4 v[LM_UNROLL];
#pragma unroll
      for (int u = 0; u < LM_UNROLL; ++u) v[u] = load4(x + 4 * (int64_t)min(c0 + u * LM_THREADS, nvec - 1));
#pragma unroll
      for (int u = 0; u < LM_UNROLL; ++u)
        if (c0 + u * LM_THREADS < nvec) ms_add4(a, v[u]);
    }
    if (tid == 0)
      for (int i = 4 * nvec; i < V; ++i) ms_add(a, x[i]);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) a = ms_merge(a, MaxSum{__shfl_xor(a.m, o, 64), __shfl_xor(a.s, o, 64)});
    if ((tid & 63) == 0) {
      wave_m[tid >> 6] = a.m;
      wave_s[tid >> 6] = a.s;
    }
    __syncthreads();
    if (tid == 0) {
      MaxSum r{wave_m[0], wave_s[0]};
      for (int w = 1; w < LM_THREADS / 64; ++w) r = ms_merge(r, MaxSum{wave_m[w], wave_s[w]});
      // lse = m + log s as an fp32 pair (value, rounding residual): at logits near 1e4 one fp32 holds it to 5e-4 only, fifty
      // times the bar on the probabilities the backward forms from it
      const float l = logf(r.s), hi = r.m + l, bb = hi - r.m, lo = (r.m - (hi - bb)) + (l - bb);
      lse[row] = hi;
      lse[rows + row] = lo;
      const int64_t lab = row_label(labels, row, T, shift, ignore);
      float out = 0.f;
      if (lab != ignore) out = (lab >= 0 && lab < V) ? (r.m - x[lab]) + l : __builtin_nanf("");
      nll[row] = out;
    }
    __syncthreads();
  }
}

// loss[0] = sum of nll over the counted rows, loss[1] = that / count, count[0] = the counted rows.  One workgroup; thread i sums
// rows i, i + 1024, ... in double, then a tree over the threads: the order is a function of `rows` alone.
__global__ __launch_bounds__(LM_REDUCE_THREADS) void lm_cross_entropy_reduce_kernel(const float* __restrict__ nll,
                                                                                    const int64_t* __restrict__ labels,
                                                                                    int64_t rows, int T, int shift, int64_t ignore,
                                                                                    float* __restrict__ loss,
                                                                                    int64_t* __restrict__ count) {
  __shared__ double part_sum[LM_REDUCE_THREADS];
  __shared__ int part_cnt[LM_REDUCE_THREADS];
  const int tid = threadIdx.x;
  double sum = 0.0;
  int cnt = 0;
  for (int64_t row = tid; row < rows; row += LM_REDUCE_THREADS)
    if (row_label(labels, row, T, shift, ignore) != ignore) {
      sum += (double)nll[row];
      ++cnt;
    }
  part_sum[tid] = sum;
  part_cnt[tid] = cnt;
  __syncthreads();
  for (int half = LM_REDUCE_THREADS / 2; half > 0; half >>= 1) {
    if (tid < half) {
      part_sum[tid] += part_sum[tid + half];
      part_cnt[tid] += part_cnt[tid + half];
    }
    __syncthreads();
  }
  if (tid == 0) {
    loss[0] = (float)part_sum[0];
    loss[1] = (float)(part_sum[0] / (double)part_cnt[0]);      // 0 / 0 = NaN when no row counts, as torch gives
    count[0] = part_cnt[0];
  }
}

// g * (exp(x - lse) - [index == lab]) of one element
__device__ __forceinline__ float lm_grad(float x, float hi, float lo, float g, int index, int lab) {
  return g * (__expf((x - hi) - lo) - (index == lab ? 1.f : 0.f));
}

__global__ __launch_bounds__(LM_THREADS) void lm_cross_entropy_bwd_kernel(const float* __restrict__ logits,
                                                                          const int64_t* __restrict__ labels,
                                                                          const float* __restrict__ lse, int64_t rows, int T, int V,
                                                                          int shift, int64_t ignore, const float* __restrict__ grad,
                                                                          const float* __restrict__ grad_per_row,
                                                                          const int64_t* __restrict__ count,
                                                                          float* __restrict__ dlogits) {
  const int tid = threadIdx.x, nvec = V >> 2;
  for (int64_t row = blockIdx.x; row < rows; row += gridDim.x) {
    const float* x = logits + row * V;
    float* d = dlogits + row * V;
    const int64_t label = row_label(labels, row, T, shift, ignore);
    if (label == ignore) {                                     // not counted: exact zeros, the logits are not read
      const float4 zero = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma clang loop vectorize(disable) interleave(disable)      // (it split the 16-byte stores into dwords)
      for (int c = tid; c < nvec; c += LM_THREADS) store4(d + 4 * (int64_t)c, zero);
      if (tid == 0)
        for (int i = 4 * nvec; i < V; ++i) d[i] = 0.f;
      continue;
    }
    float g;
    if (grad_per_row) g = grad_per_row[(row / T) * (T - shift) + row % T];
    else g = count ? grad[0] / (float)count[0] : grad[0];
    const bool in_range = label >= 0 && label < V;
    if (!in_range) g = __builtin_nanf("");                     // the forward gave this row NaN; so does the backward
    const int lab = in_range ? (int)label : -1;
    const float hi = lse[row], lo = lse[rows + row];
    for (int c0 = tid; c0 < nvec; c0 += LM_THREADS * LM_UNROLL) {
      float4 v[LM_UNROLL];
#pragma unroll
      for (int u = 0; u < LM_UNROLL; ++u) v[u] = load4(x + 4 * (int64_t)min(c0 + u * LM_THREADS, nvec - 1));
#pragma unroll
      for (int u = 0; u < LM_UNROLL; ++u) {
        const int c = c0 + u * LM_THREADS;
        if (c < nvec) {
          float4 r;
          r.x = lm_grad(v[u].x, hi, lo, g, 4 * c, lab);
          r.y = lm_grad(v[u].y, hi, lo, g, 4 * c + 1, lab);
          r.z = lm_grad(v[u].z, hi, lo, g, 4 * c + 2, lab);
          r.w = lm_grad(v[u].w, hi, lo, g, 4 * c + 3, lab);
          store4(d + 4 * (int64_t)c, r);
        }
      }
    }
    if (tid == 0)
      for (int i = 4 * nvec; i < V; ++i) d[i] = lm_grad(x[i], hi, lo, g, i, lab);
  }
}

bool aligned_to(const void* p, uintptr_t a) { return (reinterpret_cast<uintptr_t>(p) & (a - 1)) == 0; }

// nullptr when the shape is served, else the reason
const char* lm_loss_refusal(int64_t B, int64_t T, int64_t V) {
  if (B < 1 || T < 1 || V < 1) return "B, T and V must be at least 1";
  if (T >= ((int64_t)1 << 31) || V >= ((int64_t)1 << 31) || B >= ((int64_t)1 << 31) || B * T >= ((int64_t)1 << 31))
    return "problem too large for one launch (B * T and V must stay below 2^31)";
  return nullptr;
}

}  // namespace
}  // namespace spq

extern "C" int spq_lm_cross_entropy_fwd(const float* logits, const int64_t* labels, int64_t B, int64_t T, int64_t V, int shift,
                                        int64_t ignore_index, float* nll, float* lse, float* loss, int64_t* count,
                                        spq_stream_t stream) {
  using namespace spq;
  const char* null_arg = !logits ? "logits" : !labels ? "labels" : !nll ? "nll" : !lse ? "lse" : !loss ? "loss" : !count ? "count" : nullptr;
  SPQ_REQUIRE(!null_arg, "spq_lm_cross_entropy_fwd: null pointer (%s)", null_arg);
  // validate everything, then launch (DESIGN.md 3.3 "host side"): a refusal enqueues nothing
  const char* why = lm_loss_refusal(B, T, V);
  if (!why && shift != 0 && shift != 1) why = "shift must be 0 or 1";
  if (!why && !aligned_to(logits, 4)) why = "logits must be 4-byte aligned";
  if (!why && !aligned_to(labels, 8)) why = "labels must be 8-byte aligned";
  if (!why && !(aligned_to(nll, 4) && aligned_to(lse, 4) && aligned_to(loss, 4))) why = "nll, lse and loss must be 4-byte aligned";
  if (!why && !aligned_to(count, 8)) why = "count must be 8-byte aligned";
  if (why) {
    set_error("spq_lm_cross_entropy_fwd: %s (B=%lld T=%lld V=%lld shift=%d)", why, (long long)B, (long long)T, (long long)V, shift);
    return SPQ_ERR_UNSUPPORTED;
  }
  const int64_t rows = B * T;
  hipStream_t st = (hipStream_t)stream;
  const unsigned grid = (unsigned)(rows < LM_MAX_GRID ? rows : LM_MAX_GRID);
  lm_cross_entropy_fwd_kernel<<<grid, LM_THREADS, 0, st>>>(logits, labels, rows, (int)T, (int)V, shift, ignore_index, nll, lse);
  int rc = check_launch("spq_lm_cross_entropy_fwd (rows)");
  if (rc) return rc;
  lm_cross_entropy_reduce_kernel<<<1, LM_REDUCE_THREADS, 0, st>>>(nll, labels, rows, (int)T, shift, ignore_index, loss, count);
  return check_launch("spq_lm_cross_entropy_fwd (sum)");
}

extern "C" int spq_lm_cross_entropy_bwd(const float* logits, const int64_t* labels, const float* lse, int64_t B, int64_t T,
                                        int64_t V, int shift, int64_t ignore_index, const float* grad, const float* grad_per_row,
                                        const int64_t* count, float* dlogits, spq_stream_t stream) {
  using namespace spq;
  const char* null_arg = !logits ? "logits" : !labels ? "labels" : !lse ? "lse" : !dlogits ? "dlogits"
                         : (!grad && !grad_per_row) ? "grad and grad_per_row" : nullptr;
  SPQ_REQUIRE(!null_arg, "spq_lm_cross_entropy_bwd: null pointer (%s)", null_arg);
  const char* why = lm_loss_refusal(B, T, V);
  if (!why && shift != 0 && shift != 1) why = "shift must be 0 or 1";
  if (!why && grad && grad_per_row) why = "grad and grad_per_row exclude each other";
  if (!why && !(aligned_to(logits, 4) && aligned_to(dlogits, 4))) why = "logits and dlogits must be 4-byte aligned";
  if (!why && !aligned_to(labels, 8)) why = "labels must be 8-byte aligned";
  if (!why && !(aligned_to(lse, 4) && aligned_to(grad, 4) && aligned_to(grad_per_row, 4)))
    why = "lse, grad and grad_per_row must be 4-byte aligned";
  if (!why && !aligned_to(count, 8)) why = "count must be 8-byte aligned";
  if (why) {
    set_error("spq_lm_cross_entropy_bwd: %s (B=%lld T=%lld V=%lld shift=%d)", why, (long long)B, (long long)T, (long long)V, shift);
    return SPQ_ERR_UNSUPPORTED;
  }
  const int64_t rows = B * T;
  const unsigned grid = (unsigned)(rows < LM_MAX_GRID ? rows : LM_MAX_GRID);
  lm_cross_entropy_bwd_kernel<<<grid, LM_THREADS, 0, (hipStream_t)stream>>>(logits, labels, lse, rows, (int)T, (int)V, shift,
                                                                            ignore_index, grad, grad_per_row, count, dlogits);
  return check_launch("spq_lm_cross_entropy_bwd");
}
