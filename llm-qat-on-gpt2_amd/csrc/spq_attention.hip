// Causal softmax attention core on the fp32-input matrix cores (v_mfma_f32_32x32x2_f32), forward, flash style.
//
//   out[b, t, h*D + :] = softmax_j<=t( q[b,t,h] . k[b,j,h] / sqrt(D) ) . v[b,j,h]        (models_sp.py:61-75)
//
// read straight from c_attn's output qkv [B*T, 3C] (q | k | v, head h at columns h*D of each third) and written with the heads
// already merged, out [B*T, C]: no transposed copy, no T x T matrix in memory.
//
// Tile plan (operand maps and LDS images: spq_attention_tile.h).  One workgroup = 128 consecutive queries of one (sequence, head);
// wavefront w owns queries q0 + 32w .. q0 + 32w + 31.  Key tiles are 32 keys wide and anchored at position 0 (tile kt = keys
// 32kt .. 32kt + 31), so which keys meet in one MFMA and in which order they are summed is a function of the key index alone --
// not of T, B or the launch.  Per key tile a wavefront runs
//   S^T = K . Q^T          A = the K tile as a "rows" image, B = Q^T held in D/2 registers for the whole kernel
//   online softmax in fp32 on those 16 scores per lane: the row maximum and sum meet across the two lane halves with one
//                          lane ^ 32 exchange; the query's 16 probabilities stay in the registers they were born in
//   O^T += V^T . P^T       B = those registers as they are, A = the V tile as a "cols" image.  P never goes through LDS.
// Key tiles above a wavefront's diagonal are skipped; only the diagonal tile is masked (score -> -inf, probability exactly 0).
// The next tile's global loads are in flight under the current tile's MFMAs (registers -> LDS at the top of the next iteration,
// like spq_gemm_f32.hip).  Long query tiles -- the ones with the most key tiles -- get the first workgroup indices.
//
// Properties: no atomics, one fixed summation order per row; row (b, t) is computed from rows <= 32 ceil((t+1)/32)
// of its own sequence only, of which the ones above t enter as exact-zero products -- so its bits do not depend on B, on the
// position of the sequence in the batch or on T.  A NaN in q-row t makes row t NaN; a NaN in k-row j makes rows >= j NaN.  A
// non-finite v-row j makes rows >= j NaN / Inf as in the formula and, because 0 * NaN is NaN inside the diagonal tile's
// product, also the rows below j of j's own key tile (32 floor(j/32) .. j-1); the explicit formula's dense product spreads it
// to every row of the head.
#include <math.h>

#include "spq_attention_tile.h"

namespace spq {

struct AttArgs {
  const float* qkv; float* out; float* lse;
  int T, H, BH, n_qt;
  float sqrt_d;
};

template <int D>
__global__ __launch_bounds__(256, (D <= 64 ? 2 : 1)) void causal_attention_fwd_kernel(AttArgs g) {
  constexpr int HALF = D / 2, KLD = D + 4, NDB = (D + 31) / 32;
  constexpr bool POW2 = att_scale_is_pow2(D);
  __shared__ __attribute__((aligned(16))) float Ks[ATT_TILE * KLD];
  __shared__ __attribute__((aligned(16))) float Vt[NDB * 32 * ATT_TLD];
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, l31 = lane & 31, h = lane >> 5;
  const int T = g.T;
  const AttWork wk = att_work(g.n_qt, true, g.BH, g.H, D, T, w);           // long query tiles first
  const int qt = wk.blk;
  const int64_t C = wk.C, ld = wk.ld;
  const float* base = g.qkv + (int64_t)wk.b * T * ld + (int64_t)wk.hd * D;
  const float* kbase = base + C;
  const float* vbase = base + 2 * C;
  const int qrow = wk.row0 + l31;
  const int kt_last = min(qt * (ATT_BLOCK / ATT_TILE) + (ATT_BLOCK / ATT_TILE - 1), (T - 1) / ATT_TILE);

  float q[HALF];
  att_load_half_row<D>(q, base + (int64_t)min(qrow, T - 1) * ld + HALF * h, POW2 ? 1.0f / g.sqrt_d : 1.0f);

  att_f32x16 acc[NDB];
  att_zero(acc);
  float m = -INFINITY, l = 0.f;                  // running maximum (of the whole row) and this lane half's share of the sum

  AttRows<D> rk;
  AttCols<D> cv;
  att_load_rows<D>(rk, kbase, ld, 0, T, tid);
  att_load_cols<D>(cv, vbase, ld, 0, T, tid);
  for (int kt = 0; kt <= kt_last; ++kt) {
    __syncthreads();                             // the previous tile's fragment reads are done
    att_store_rows<D>(rk, Ks, tid);
    att_store_cols<D>(cv, Vt, tid);
    __syncthreads();
    if (kt < kt_last) {
      att_load_rows<D>(rk, kbase, ld, (kt + 1) * ATT_TILE, T, tid);
      att_load_cols<D>(cv, vbase, ld, (kt + 1) * ATT_TILE, T, tid);
    }
    if (!wk.active || kt > wk.diag) continue;    // above this wavefront's diagonal (it still moves tiles for the others)

    // ---- S^T = K . Q^T: register e of lane half h = key 4h + (e & 3) + 8 (e >> 2), lane & 31 = query
    att_f32x16 s = att_rows_times_regs<D>(Ks + l31 * KLD + HALF * h, q);
    if (!POW2) {
#pragma unroll
      for (int e = 0; e < 16; ++e) s[e] = s[e] / g.sqrt_d;                  // models_sp.py:68
    }
    if (kt == wk.diag) {                                                     // the diagonal tile: its first key is this wavefront's first query
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
    att_cols_times_cd<NDB>(acc, Vt + l31 * ATT_TLD + 4 * h, s);
  }

  if (!wk.active) return;
  const float lt = l + __shfl_xor(l, 32, 64);   // (commutative: both halves hold the same bits)
  if (qrow >= T) return;
  att_store_acc<D, NDB, false>(acc, g.out + ((int64_t)wk.b * T + qrow) * C + (int64_t)wk.hd * D, h, 1.0f, lt);
  if (g.lse && h == 0) g.lse[(int64_t)wk.bh * T + qrow] = m + logf(lt);
}

template <int D>
static int launch_attention(const AttArgs& g, unsigned grid, hipStream_t st) {
  causal_attention_fwd_kernel<D><<<grid, 256, 0, st>>>(g);
  return check_launch("spq_causal_attention_fwd");
}

// The backward serves fewer head sizes and bounds B by itself as well.
const char* attention_refusal(int64_t B, int64_t T, int64_t n_head, int64_t head_dim, bool backward) {
  const bool dim_ok = head_dim == 16 || head_dim == 32 || head_dim == 64 || (!backward && (head_dim == 80 || head_dim == 128));
  if (!dim_ok) return backward ? "head_dim must be 64 (or 16, 32)" : "head_dim must be 64 (or 16, 32, 80, 128)";
  if (B < 1 || T < 1 || n_head < 1) return "B, T and n_head must be at least 1";
  const int64_t n_blk = (T + ATT_BLOCK - 1) / ATT_BLOCK;
  if (T >= (1 << 24) || n_head >= (1 << 16) || (backward && B >= ((int64_t)1 << 31)) || B * n_head * n_blk >= ((int64_t)1 << 31))
    return "problem too large for one launch";
  return nullptr;
}

}  // namespace spq

extern "C" int spq_causal_attention_fwd(const float* qkv, int64_t B, int64_t T, int64_t n_head, int64_t head_dim, float* out,
                                        float* lse, spq_stream_t stream) {
  using namespace spq;
  SPQ_REQUIRE(qkv && out, "spq_causal_attention_fwd: null pointer");
  // validate everything, then launch (DESIGN.md 3.3 "host side"): a refusal enqueues nothing
  const char* why = attention_refusal(B, T, n_head, head_dim, false);
  if (!why && (!aligned16(qkv) || !aligned16(out) || (lse && !aligned16(lse)))) why = "pointers must be 16-byte aligned";
  if (why) {
    set_error("spq_causal_attention_fwd: %s (B=%lld T=%lld n_head=%lld head_dim=%lld)", why, (long long)B, (long long)T,
              (long long)n_head, (long long)head_dim);
    return SPQ_ERR_UNSUPPORTED;
  }
  const int64_t n_qt = (T + ATT_BLOCK - 1) / ATT_BLOCK;
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
