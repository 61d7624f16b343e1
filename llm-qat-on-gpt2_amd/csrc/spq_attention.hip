// Causal softmax attention core on the fp32-input matrix cores (v_mfma_f32_32x32x2_f32), forward, flash style.
//
//   out[b, t, h*D + :] = softmax_j<=t( q[b,t,h] . k[b,j,h] / sqrt(D) ) . v[b,j,h]        (models_sp.py:61-75)
//
// read straight from c_attn's output qkv [B*T, 3C] (q | k | v, head h at columns h*D of each third) and written with the heads
// already merged, out [B*T, C]: no transposed copy, no T x T matrix in memory.
//
// Tile plan.  One 256-thread workgroup = 128 consecutive queries of one (sequence, head); wavefront w owns queries
// q0 + 32w .. q0 + 32w + 31.  Key tiles are 32 keys wide and ANCHORED AT POSITION 0 (tile kt = keys 32kt .. 32kt + 31), so which
// keys meet in one MFMA and in which order they are summed is a function of the key index alone -- not of T, B or the launch.
// Per key tile a wavefront runs
//   S^T = K . Q^T          A = K tile from LDS [key][D + 4] (lane half h reads the D/2 contiguous d of its key row with
//                          ds_read_b128; k index of step s = d (D/2)h + s), B = Q^T held in D/2 registers for the whole kernel
//                          in that same d order.  C/D map of the 32x32 MFMA: lane = query (lane & 31), register r of lane
//                          half h = key kk(r, h) = 4h + (r & 3) + 8 (r >> 2).
//   online softmax in fp32 on those 16 scores per lane: the row maximum and sum meet across the two lane halves with one
//                          lane ^ 32 exchange; the query's 16 probabilities stay in the registers they were born in
//   O^T += V^T . P^T       B = those registers as they are (step r sums keys kk(r, 0), kk(r, 1)), A = V^T from an LDS image
//                          [d][32 keys + 4] written transposed, so lane (d, h) reads keys kk(4g .. 4g+3, h) of step group g as ONE
//                          ds_read_b128.  P never goes through LDS.
// Key tiles above a wavefront's diagonal are skipped; only the diagonal tile is masked (score -> -inf, probability exactly 0).
// Rows of K and V at positions >= T are loaded as zeros.  The next tile's global loads are in flight under the current tile's
// MFMAs (registers -> LDS at the top of the next iteration, like spq_gemm_f32.hip).  Long query tiles -- the ones with the most
// key tiles -- get the first workgroup indices.
//
// Properties: no atomics, one fixed summation order per row; row (b, t) is computed from rows <= 32 ceil((t+1)/32)
// of its own sequence only, of which the ones above t enter as exact-zero products -- so its bits do not depend on B, on the
// position of the sequence in the batch or on T.  A NaN in q-row t makes row t NaN; a NaN in k-row j makes rows >= j NaN.  A
// non-finite v-row j makes rows >= j NaN / Inf as in the formula and, because 0 * NaN is NaN inside the diagonal tile's
// product, also the rows below j of j's own key tile (32 floor(j/32) .. j-1); the explicit formula's dense product spreads it
// to every row of the head.
#include <math.h>

#include "spq_common.h"

namespace spq {

typedef float att_f32x16 __attribute__((ext_vector_type(16)));

constexpr int ATT_BQ = 128, ATT_BK = 32, ATT_VLD = ATT_BK + 4;

struct AttArgs {
  const float* qkv; float* out; float* lse;
  int T, H, BH, n_qt;
  float sqrt_d;
};

// one key tile on its way global -> registers -> LDS: K as float4 along d, V as 4 consecutive keys of one d
template <int D>
struct AttTileRegs {
  static constexpr int NK = (ATT_BK * D / 4 + 255) / 256, NV = (D * (ATT_BK / 4) + 255) / 256;
  float4 k[NK], v[NV];
};

template <int D>
__device__ __forceinline__ void att_load_tile(AttTileRegs<D>& r, const float* __restrict__ kbase, const float* __restrict__ vbase,
                                              int64_t ld, int k0, int T, int tid) {
#pragma unroll
  for (int i = 0; i < AttTileRegs<D>::NK; ++i) {
    const int idx = tid + 256 * i;
    const int key = idx / (D / 4), c = (idx % (D / 4)) * 4;
    float4 val = make_float4(0.f, 0.f, 0.f, 0.f);
    if (idx < ATT_BK * D / 4 && k0 + key < T) val = *reinterpret_cast<const float4*>(kbase + (int64_t)(k0 + key) * ld + c);
    r.k[i] = val;
  }
#pragma unroll
  for (int i = 0; i < AttTileRegs<D>::NV; ++i) {
    const int idx = tid + 256 * i;
    const int d = idx % D, key = k0 + (idx / D) * 4;
    float4 val = make_float4(0.f, 0.f, 0.f, 0.f);
    if (idx < D * (ATT_BK / 4)) {
      const float* p = vbase + (int64_t)key * ld + d;
      if (key + 0 < T) val.x = p[0];
      if (key + 1 < T) val.y = p[ld];
      if (key + 2 < T) val.z = p[2 * ld];
      if (key + 3 < T) val.w = p[3 * ld];
    }
    r.v[i] = val;
  }
}

template <int D>
__device__ __forceinline__ void att_store_tile(const AttTileRegs<D>& r, float* __restrict__ Ks, float* __restrict__ Vt, int tid) {
#pragma unroll
  for (int i = 0; i < AttTileRegs<D>::NK; ++i) {
    const int idx = tid + 256 * i;
    if (idx < ATT_BK * D / 4) *reinterpret_cast<float4*>(Ks + (idx / (D / 4)) * (D + 4) + (idx % (D / 4)) * 4) = r.k[i];
  }
#pragma unroll
  for (int i = 0; i < AttTileRegs<D>::NV; ++i) {
    const int idx = tid + 256 * i;
    if (idx < D * (ATT_BK / 4)) *reinterpret_cast<float4*>(Vt + (idx % D) * ATT_VLD + (idx / D) * 4) = r.v[i];
  }
}

template <int D>
__global__ __launch_bounds__(256, (D <= 64 ? 2 : 1)) void causal_attention_fwd_kernel(AttArgs g) {
  constexpr int HALF = D / 2, KLD = D + 4, NDB = (D + 31) / 32;
  // 1 / sqrt(D) is a power of two for D = 16, 64: scaling q by it is then the reference's division of the score, bit for bit
  constexpr bool POW2 = (D == 16 || D == 64);
  __shared__ __attribute__((aligned(16))) float Ks[ATT_BK * KLD];
  __shared__ __attribute__((aligned(16))) float Vt[NDB * 32 * ATT_VLD];   // rows >= D (D = 16, 80) are never written: they feed only
                                                                          // the output rows >= D, which are never stored
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, l31 = lane & 31, h = lane >> 5;
  const int qt = g.n_qt - 1 - (int)(blockIdx.x / (unsigned)g.BH);         // long query tiles first
  const int bh = (int)(blockIdx.x % (unsigned)g.BH);
  const int b = bh / g.H, hd = bh % g.H;
  const int T = g.T;
  const int64_t C = (int64_t)g.H * D, ld = 3 * C;
  const float* base = g.qkv + (int64_t)b * T * ld + (int64_t)hd * D;
  const float* kbase = base + C;
  const float* vbase = base + 2 * C;

  const int qw0 = qt * ATT_BQ + 32 * w;          // first query of this wavefront; its diagonal key tile starts there too
  const int qrow = qw0 + l31;
  const bool active = qw0 < T;                   // wavefront-uniform
  const int my_diag = qw0 / ATT_BK;
  const int kt_last = min(qt * (ATT_BQ / ATT_BK) + (ATT_BQ / ATT_BK - 1), (T - 1) / ATT_BK);

  float q[HALF];
  {
    const float* qp = base + (int64_t)min(qrow, T - 1) * ld + HALF * h;
    const float qs = POW2 ? 1.0f / g.sqrt_d : 1.0f;
#pragma unroll
    for (int i = 0; i < HALF / 4; ++i) {
      const float4 v4 = *reinterpret_cast<const float4*>(qp + 4 * i);
      q[4 * i + 0] = v4.x * qs; q[4 * i + 1] = v4.y * qs; q[4 * i + 2] = v4.z * qs; q[4 * i + 3] = v4.w * qs;
    }
  }

  att_f32x16 acc[NDB];
#pragma unroll
  for (int i = 0; i < NDB; ++i)
#pragma unroll
    for (int e = 0; e < 16; ++e) acc[i][e] = 0.f;
  float m = -INFINITY, l = 0.f;                  // running maximum (of the whole row) and this lane half's share of the sum

  AttTileRegs<D> regs;
  att_load_tile<D>(regs, kbase, vbase, ld, 0, T, tid);
  for (int kt = 0; kt <= kt_last; ++kt) {
    __syncthreads();                             // the previous tile's fragment reads are done
    att_store_tile<D>(regs, Ks, Vt, tid);
    __syncthreads();
    if (kt < kt_last) att_load_tile<D>(regs, kbase, vbase, ld, (kt + 1) * ATT_BK, T, tid);
    if (!active || kt > my_diag) continue;       // above this wavefront's diagonal (it still moves tiles for the others)

    // ---- S^T = K . Q^T
    att_f32x16 s;
#pragma unroll
    for (int e = 0; e < 16; ++e) s[e] = 0.f;
    const float* kp = Ks + l31 * KLD + HALF * h;
#pragma unroll
    for (int i = 0; i < HALF / 4; ++i) {
      const float4 kv = *reinterpret_cast<const float4*>(kp + 4 * i);
      s = __builtin_amdgcn_mfma_f32_32x32x2f32(kv.x, q[4 * i + 0], s, 0, 0, 0);
      s = __builtin_amdgcn_mfma_f32_32x32x2f32(kv.y, q[4 * i + 1], s, 0, 0, 0);
      s = __builtin_amdgcn_mfma_f32_32x32x2f32(kv.z, q[4 * i + 2], s, 0, 0, 0);
      s = __builtin_amdgcn_mfma_f32_32x32x2f32(kv.w, q[4 * i + 3], s, 0, 0, 0);
    }
    if (!POW2) {
#pragma unroll
      for (int e = 0; e < 16; ++e) s[e] = s[e] / g.sqrt_d;                  // models_sp.py:68
    }
    if (kt == my_diag) {                                                    // the diagonal tile: its first key is this wavefront's first query
#pragma unroll
      for (int e = 0; e < 16; ++e)
        if (4 * h + (e & 3) + 8 * (e >> 2) > l31) s[e] = -INFINITY;         // :70 (also replaces a NaN score of a masked key)
    }

    // ---- online softmax: fmaxf drops a NaN score, exp() then carries it into the sum
    float mt = s[0];
#pragma unroll
    for (int e = 1; e < 16; ++e) mt = fmaxf(mt, s[e]);
    mt = fmaxf(mt, __shfl_xor(mt, 32, 64));
    const float m_new = fmaxf(m, mt);
    const float alpha = expf(m - m_new);
    float ps = 0.f;
#pragma unroll
    for (int e = 0; e < 16; ++e) {
      s[e] = expf(s[e] - m_new);
      ps += s[e];
    }
    l = l * alpha + ps;
    m = m_new;
#pragma unroll
    for (int i = 0; i < NDB; ++i)
#pragma unroll
      for (int e = 0; e < 16; ++e) acc[i][e] *= alpha;

    // ---- O^T += V^T . P^T
    const float* vp = Vt + l31 * ATT_VLD + 4 * h;
#pragma unroll
    for (int gi = 0; gi < 4; ++gi) {
#pragma unroll
      for (int i = 0; i < NDB; ++i) {
        const float4 vv = *reinterpret_cast<const float4*>(vp + i * 32 * ATT_VLD + 8 * gi);
        acc[i] = __builtin_amdgcn_mfma_f32_32x32x2f32(vv.x, s[4 * gi + 0], acc[i], 0, 0, 0);
        acc[i] = __builtin_amdgcn_mfma_f32_32x32x2f32(vv.y, s[4 * gi + 1], acc[i], 0, 0, 0);
        acc[i] = __builtin_amdgcn_mfma_f32_32x32x2f32(vv.z, s[4 * gi + 2], acc[i], 0, 0, 0);
        acc[i] = __builtin_amdgcn_mfma_f32_32x32x2f32(vv.w, s[4 * gi + 3], acc[i], 0, 0, 0);
      }
    }
  }

  if (!active) return;
  const float lt = l + __shfl_xor(l, 32, 64);   // (commutative: both halves hold the same bits)
  if (qrow >= T) return;
  float* op = g.out + ((int64_t)b * T + qrow) * C + (int64_t)hd * D;
#pragma unroll
  for (int i = 0; i < NDB; ++i) {
#pragma unroll
    for (int gi = 0; gi < 4; ++gi) {
      const int dd = i * 32 + 8 * gi + 4 * h;    // rows (e & 3) + 8 (e >> 2) + 4h of the C/D map, e = 4 gi .. 4 gi + 3
      if (dd < D)
        *reinterpret_cast<float4*>(op + dd) = make_float4(acc[i][4 * gi + 0] / lt, acc[i][4 * gi + 1] / lt,
                                                          acc[i][4 * gi + 2] / lt, acc[i][4 * gi + 3] / lt);
    }
  }
  if (g.lse && h == 0) g.lse[(int64_t)bh * T + qrow] = m + logf(lt);
}

template <int D>
static int launch_attention(const AttArgs& g, unsigned grid, hipStream_t st) {
  causal_attention_fwd_kernel<D><<<grid, 256, 0, st>>>(g);
  return check_launch("spq_causal_attention_fwd");
}

}  // namespace spq

extern "C" int spq_causal_attention_fwd(const float* qkv, int64_t B, int64_t T, int64_t n_head, int64_t head_dim, float* out,
                                        float* lse, spq_stream_t stream) {
  using namespace spq;
  SPQ_REQUIRE(qkv && out, "spq_causal_attention_fwd: null pointer");
  // validate everything, then launch (DESIGN.md 3.3 "host side"): a refusal enqueues nothing
  const bool dim_ok = head_dim == 16 || head_dim == 32 || head_dim == 64 || head_dim == 80 || head_dim == 128;
  const int64_t n_qt = T > 0 ? (T + ATT_BQ - 1) / ATT_BQ : 0;
  const char* why = nullptr;
  if (!dim_ok) why = "head_dim must be 64 (or 16, 32, 80, 128)";
  else if (B < 1 || T < 1 || n_head < 1) why = "B, T and n_head must be at least 1";
  else if (T >= (1 << 24) || n_head >= (1 << 16) || B * n_head * n_qt >= ((int64_t)1 << 31)) why = "problem too large for one launch";
  else if (!aligned16(qkv) || !aligned16(out) || (lse && !aligned16(lse))) why = "pointers must be 16-byte aligned";
  if (why) {
    set_error("spq_causal_attention_fwd: %s (B=%lld T=%lld n_head=%lld head_dim=%lld)", why, (long long)B, (long long)T,
              (long long)n_head, (long long)head_dim);
    return SPQ_ERR_UNSUPPORTED;
  }
  AttArgs g;
  g.qkv = qkv; g.out = out; g.lse = lse;
  g.T = (int)T; g.H = (int)n_head; g.BH = (int)(B * n_head); g.n_qt = (int)n_qt;
  g.sqrt_d = (float)sqrt((double)head_dim);
  const unsigned grid = (unsigned)(B * n_head * n_qt);
  hipStream_t st = (hipStream_t)stream;
  switch (head_dim) {
    case 16: return launch_attention<16>(g, grid, st);
    case 32: return launch_attention<32>(g, grid, st);
    case 64: return launch_attention<64>(g, grid, st);
    case 80: return launch_attention<80>(g, grid, st);
    default: return launch_attention<128>(g, grid, st);
  }
}
