// Backward of the causal softmax attention core (spq_attention.hip) on the same fp32-input MFMA (v_mfma_f32_32x32x2_f32),
// recomputing the probabilities from the forward's log-sum-exp.  For one (sequence, head), s = q k^T / sqrt(D) masked causally:
//
//   P = exp(s - lse)     delta_i = sum_d dO_i O_i     dV_j = sum_{i>=j} P_ij dO_i     dP_ij = dO_i . V_j
//   dS_ij = P_ij (dP_ij - delta_i)     dQ_i = sum_{j<=i} dS_ij K_j / sqrt(D)     dK_j = sum_{i>=j} dS_ij Q_i / sqrt(D)
//
// qkv [B*T, 3C] is read where it lies, dout / out [B*T, C] with the heads merged, and dqkv [B*T, 3C] = dq | dk | dv is written in
// c_attn's own layout: no transposed copy, no cat, no T x T matrix in memory.  Three launches on the forward's tile plan (operand
// maps and the "rows" / "cols" LDS images: spq_attention_tile.h):
//
//   delta    the diagonal of O . dO^T, 32 rows per wavefront on the MFMA in the summation order of dP -> workspace [B, H, T].
//   dQ       mirrors the forward.  One 256-thread workgroup = 128 queries, wavefront w owns 32 of them (lane & 31 = query) and
//            walks the 32-key tiles, anchored at position 0, up to its diagonal.  Q^T and dO^T stay in registers as the B operands
//            of S^T = K . Q^T and dP^T = V . dO^T (A = the K / V tile as a "rows" image); dS^T is born in the C/D registers
//            and is, as it is, the B operand of dQ^T += K^T . dS^T (A = the K tile as a "cols" image).
//   dK/dV    the same plan with the roles swapped.  A workgroup owns 128 keys, wavefront w 32 of them (lane & 31 = key) with
//            K^T and V^T in registers, and walks the 32-query tiles, anchored at position 0, from its diagonal to the end:
//            S = Q . K^T and dP = dO . V^T (A = the Q / dO tile as a "rows" image), then dV^T += dO^T . P and
//            dK^T += Q^T . dS with A from the "cols" images and B = the registers P / dS were born in.  lse and delta of
//            the tile's 32 queries go through LDS.  The first workgroup indices get the first key tiles: the longest walks.
//
// Only the diagonal tile is masked: there P and dS are forced to exactly 0 (not left to exp of -inf times something).  Rows at
// positions >= T are loaded as zeros and, in the dK/dV walk, their P and dS are forced to 0 as well -- lse is never read there.
//
// Properties: no atomics; every element of dqkv is written; one fixed summation order per output element that is
// a function of the query / key index alone (tiles anchored at 0 along both axes), so the bits do not depend on B, on the place
// of the sequence in the batch or on the grid, and runs repeat bit for bit.  (b, h) pairs never meet: a NaN stays in its head.
#include <math.h>

#include "spq_attention_tile.h"

namespace spq {

struct AttBwdArgs {
  const float* qkv; const float* out; const float* lse; const float* dout; const float* delta;
  float* dqkv; float* delta_out;
  int T, H, BH, n_blk;
  float sqrt_d;
};

// ---- delta[b, h, t] = sum_d dO[b, t, h D + d] O[b, t, h D + d] --------------------------------------------------------------
// The diagonal of O . dO^T on the MFMA, with O where the walks have V: delta is then summed in exactly the order of dP = dO . V^T,
// so where O is V bit for bit (a row that attends to one key) dP - delta is exactly 0.  Wavefront w = 32 rows, no LDS.
template <int D>
__global__ __launch_bounds__(256) void causal_attention_bwd_delta_kernel(AttBwdArgs g) {
  constexpr int HALF = D / 2;
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, l31 = lane & 31, h = lane >> 5;
  const int T = g.T;
  const AttWork wk = att_work(g.n_blk, false, g.BH, g.H, D, T, w);
  if (!wk.active) return;                        // wavefront-uniform; the kernel has no barrier
  const int qrow = wk.row0 + l31;
  const int64_t off = ((int64_t)wk.b * T + min(qrow, T - 1)) * wk.C + (int64_t)wk.hd * D + HALF * h;
  float o[HALF], dO[HALF];
  att_load_half_row<D>(o, g.out + off, 1.0f);
  att_load_half_row<D>(dO, g.dout + off, 1.0f);
  att_f32x16 c;
  att_zero(c);
#pragma unroll
  for (int i = 0; i < HALF; ++i) c = __builtin_amdgcn_mfma_f32_32x32x2f32(o[i], dO[i], c, 0, 0, 0);
  // row l31 of column l31 lies in register (l31 & 3) + 4 (l31 >> 3) of lane half (l31 >> 2) & 1
  const int e_mine = (l31 & 3) + 4 * (l31 >> 3);
  float mine = 0.f;
#pragma unroll
  for (int e = 0; e < 16; ++e)
    if (e == e_mine) mine = c[e];
  const float other = __shfl_xor(mine, 32, 64);
  const float delta = (((l31 >> 2) & 1) == h) ? mine : other;
  if (h == 0 && qrow < T) g.delta_out[(int64_t)wk.bh * T + qrow] = delta;
}

// ---- dQ ---------------------------------------------------------------------------------------------------------------------
template <int D>
__global__ __launch_bounds__(256, 2) void causal_attention_bwd_dq_kernel(AttBwdArgs g) {
  constexpr int HALF = D / 2, KLD = D + 4, NDB = (D + 31) / 32;
  constexpr bool POW2 = att_scale_is_pow2(D);    // as the forward: q is scaled, else the score divided
  __shared__ __attribute__((aligned(16))) float Ks[ATT_TILE * KLD];
  __shared__ __attribute__((aligned(16))) float Vs[ATT_TILE * KLD];
  __shared__ __attribute__((aligned(16))) float Kt[NDB * 32 * ATT_TLD];
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, l31 = lane & 31, h = lane >> 5;
  const int T = g.T;
  const AttWork wk = att_work(g.n_blk, true, g.BH, g.H, D, T, w);          // long query tiles first
  const int qt = wk.blk;
  const int64_t C = wk.C, ld = wk.ld;
  const float* base = g.qkv + (int64_t)wk.b * T * ld + (int64_t)wk.hd * D;
  const float* kbase = base + C;
  const float* vbase = base + 2 * C;
  const int qrow = wk.row0 + l31, qclamp = min(qrow, T - 1);
  const int kt_last = min(qt * (ATT_BLOCK / ATT_TILE) + (ATT_BLOCK / ATT_TILE - 1), (T - 1) / ATT_TILE);

  float q[HALF], dO[HALF];
  att_load_half_row<D>(q, base + (int64_t)qclamp * ld + HALF * h, POW2 ? 1.0f / g.sqrt_d : 1.0f);
  att_load_half_row<D>(dO, g.dout + ((int64_t)wk.b * T + qclamp) * C + (int64_t)wk.hd * D + HALF * h, 1.0f);
  const float lse_q = g.lse[(int64_t)wk.bh * T + qclamp];
  const float delta_q = g.delta[(int64_t)wk.bh * T + qclamp];

  att_f32x16 acc[NDB];
  att_zero(acc);

  AttRows<D> rk, rv;
  AttCols<D> ck;
  att_load_rows<D>(rk, kbase, ld, 0, T, tid);
  att_load_rows<D>(rv, vbase, ld, 0, T, tid);
  att_load_cols<D>(ck, kbase, ld, 0, T, tid);
  for (int kt = 0; kt <= kt_last; ++kt) {
    __syncthreads();                             // the previous tile's fragment reads are done
    att_store_rows<D>(rk, Ks, tid);
    att_store_rows<D>(rv, Vs, tid);
    att_store_cols<D>(ck, Kt, tid);
    __syncthreads();
    if (kt < kt_last) {
      att_load_rows<D>(rk, kbase, ld, (kt + 1) * ATT_TILE, T, tid);
      att_load_rows<D>(rv, vbase, ld, (kt + 1) * ATT_TILE, T, tid);
      att_load_cols<D>(ck, kbase, ld, (kt + 1) * ATT_TILE, T, tid);
    }
    if (!wk.active || kt > wk.diag) continue;    // above this wavefront's diagonal (it still moves tiles for the others)

    // ---- S^T = K . Q^T and dP^T = V . dO^T: register e of lane half h = key 4h + (e & 3) + 8 (e >> 2), lane & 31 = query
    att_f32x16 s = att_rows_times_regs<D>(Ks + l31 * KLD + HALF * h, q);
    const att_f32x16 dp = att_rows_times_regs<D>(Vs + l31 * KLD + HALF * h, dO);
    const bool diag = kt == wk.diag;
#pragma unroll
    for (int e = 0; e < 16; ++e) {
      const bool masked = diag && (4 * h + (e & 3) + 8 * (e >> 2) > l31);
      const float sc = POW2 ? s[e] : s[e] / g.sqrt_d;
      const float p = expf(sc - lse_q);
      s[e] = masked ? 0.f : p * (dp[e] - delta_q);                     // dS^T (exactly 0 where masked, whatever dP is)
    }
    // ---- dQ^T += K^T . dS^T
    att_cols_times_cd<NDB>(acc, Kt + l31 * ATT_TLD + 4 * h, s);
  }

  if (!wk.active || qrow >= T) return;
  att_store_acc<D, NDB, POW2>(acc, g.dqkv + ((int64_t)wk.b * T + qrow) * ld + (int64_t)wk.hd * D, h, 1.0f / g.sqrt_d, g.sqrt_d);
}

// ---- dK and dV --------------------------------------------------------------------------------------------------------------
template <int D>
__global__ __launch_bounds__(256, 1) void causal_attention_bwd_dkv_kernel(AttBwdArgs g) {
  constexpr int HALF = D / 2, KLD = D + 4, NDB = (D + 31) / 32;
  constexpr bool POW2 = att_scale_is_pow2(D);
  __shared__ __attribute__((aligned(16))) float Qs[ATT_TILE * KLD];
  __shared__ __attribute__((aligned(16))) float Gs[ATT_TILE * KLD];       // the dO tile
  __shared__ __attribute__((aligned(16))) float Qt[NDB * 32 * ATT_TLD];
  __shared__ __attribute__((aligned(16))) float Gt[NDB * 32 * ATT_TLD];
  __shared__ __attribute__((aligned(16))) float Ls[ATT_TILE];             // lse and delta of the tile's queries
  __shared__ __attribute__((aligned(16))) float Ds[ATT_TILE];

  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, l31 = lane & 31, h = lane >> 5;
  const int T = g.T;
  const AttWork wk = att_work(g.n_blk, false, g.BH, g.H, D, T, w);         // rows = keys here; first key blocks first: the longest walks
  const int kb = wk.blk;
  const int64_t C = wk.C, ld = wk.ld;
  const float* qbase = g.qkv + (int64_t)wk.b * T * ld + (int64_t)wk.hd * D;
  const float* gbase = g.dout + (int64_t)wk.b * T * C + (int64_t)wk.hd * D;
  const float* lbase = g.lse + (int64_t)wk.bh * T;
  const float* dbase = g.delta + (int64_t)wk.bh * T;
  const int krow = wk.row0 + l31, kclamp = min(krow, T - 1);
  const int qt_first = kb * (ATT_BLOCK / ATT_TILE), qt_last = (T - 1) / ATT_TILE;

  float k[HALF], v[HALF];
  att_load_half_row<D>(k, qbase + C + (int64_t)kclamp * ld + HALF * h, POW2 ? 1.0f / g.sqrt_d : 1.0f);
  att_load_half_row<D>(v, qbase + 2 * C + (int64_t)kclamp * ld + HALF * h, 1.0f);

  att_f32x16 dk[NDB], dv[NDB];
  att_zero(dk);
  att_zero(dv);

  AttRows<D> rq, rg;
  AttCols<D> cq, cg;
  float r_lse = 0.f, r_delta = 0.f;              // threads 0..31: one query's lse and delta (0 at positions >= T, never used)
  auto load_tile = [&](int q0) {
    att_load_rows<D>(rq, qbase, ld, q0, T, tid);
    att_load_rows<D>(rg, gbase, C, q0, T, tid);
    att_load_cols<D>(cq, qbase, ld, q0, T, tid);
    att_load_cols<D>(cg, gbase, C, q0, T, tid);
    if (tid < ATT_TILE) {
      const bool in = q0 + tid < T;
      r_lse = in ? lbase[q0 + tid] : 0.f;
      r_delta = in ? dbase[q0 + tid] : 0.f;
    }
  };
  load_tile(qt_first * ATT_TILE);
  for (int qt = qt_first; qt <= qt_last; ++qt) {
    __syncthreads();
    att_store_rows<D>(rq, Qs, tid);
    att_store_rows<D>(rg, Gs, tid);
    att_store_cols<D>(cq, Qt, tid);
    att_store_cols<D>(cg, Gt, tid);
    if (tid < ATT_TILE) { Ls[tid] = r_lse; Ds[tid] = r_delta; }
    __syncthreads();
    if (qt < qt_last) load_tile((qt + 1) * ATT_TILE);
    if (!wk.active || qt < wk.diag) continue;    // query tiles before this wavefront's diagonal see none of its keys

    // ---- S = Q . K^T and dP = dO . V^T: register e of lane half h = query 4h + (e & 3) + 8 (e >> 2), lane & 31 = key
    att_f32x16 s = att_rows_times_regs<D>(Qs + l31 * KLD + HALF * h, k);
    att_f32x16 dp = att_rows_times_regs<D>(Gs + l31 * KLD + HALF * h, v);
    const bool diag = qt == wk.diag;
    const int q_left = T - qt * ATT_TILE;       // queries of this tile at positions < T (>= 32 except in the last tile)
#pragma unroll
    for (int gi = 0; gi < 4; ++gi) {
      const float4 l4 = *reinterpret_cast<const float4*>(Ls + 8 * gi + 4 * h);
      const float4 d4 = *reinterpret_cast<const float4*>(Ds + 8 * gi + 4 * h);
      const float lq[4] = {l4.x, l4.y, l4.z, l4.w}, dq[4] = {d4.x, d4.y, d4.z, d4.w};
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int e = 4 * gi + j, qi = 4 * h + j + 8 * gi;
        const bool masked = (diag && l31 > qi) || qi >= q_left;
        const float sc = POW2 ? s[e] : s[e] / g.sqrt_d;
        const float p = masked ? 0.f : expf(sc - lq[j]);                // exactly 0 where masked and at positions >= T
        s[e] = p;
        dp[e] = masked ? 0.f : p * (dp[e] - dq[j]);                     // dS
      }
    }
    // ---- dV^T += dO^T . P and dK^T += Q^T . dS
    att_cols_times_cd<NDB>(dv, Gt + l31 * ATT_TLD + 4 * h, s);
    att_cols_times_cd<NDB>(dk, Qt + l31 * ATT_TLD + 4 * h, dp);
  }

  if (!wk.active || krow >= T) return;
  float* op = g.dqkv + ((int64_t)wk.b * T + krow) * ld + (int64_t)wk.hd * D;
  att_store_acc<D, NDB, POW2>(dk, op + C, h, 1.0f / g.sqrt_d, g.sqrt_d);
  att_store_acc<D, NDB, true>(dv, op + 2 * C, h, 1.0f, 1.0f);
}

template <int D>
static int launch_attention_bwd(const AttBwdArgs& g, hipStream_t st) {
  const unsigned grid = (unsigned)((int64_t)g.BH * g.n_blk);
  causal_attention_bwd_delta_kernel<D><<<grid, 256, 0, st>>>(g);
  int rc = check_launch("spq_causal_attention_bwd (delta)");
  if (rc) return rc;
  causal_attention_bwd_dq_kernel<D><<<grid, 256, 0, st>>>(g);
  rc = check_launch("spq_causal_attention_bwd (dq)");
  if (rc) return rc;
  causal_attention_bwd_dkv_kernel<D><<<grid, 256, 0, st>>>(g);
  return check_launch("spq_causal_attention_bwd (dk, dv)");
}

}  // namespace spq

extern "C" int64_t spq_causal_attention_bwd_workspace_bytes(int64_t B, int64_t T, int64_t n_head, int64_t head_dim) {
  using namespace spq;
  if (const char* why = attention_refusal(B, T, n_head, head_dim, true)) {
    set_error("spq_causal_attention_bwd_workspace_bytes: %s (B=%lld T=%lld n_head=%lld head_dim=%lld)", why, (long long)B,
              (long long)T, (long long)n_head, (long long)head_dim);
    return SPQ_ERR_UNSUPPORTED;
  }
  return (B * n_head * T * (int64_t)sizeof(float) + 15) / 16 * 16;      // delta [B, n_head, T]
}

extern "C" int spq_causal_attention_bwd(const float* qkv, const float* out, const float* lse, const float* dout, int64_t B,
                                        int64_t T, int64_t n_head, int64_t head_dim, float* dqkv, void* workspace,
                                        size_t workspace_bytes, spq_stream_t stream) {
  using namespace spq;
  SPQ_REQUIRE(qkv && out && lse && dout && dqkv && workspace, "spq_causal_attention_bwd: null pointer");
  // validate everything, then launch (DESIGN.md 3.3 "host side"): a refusal enqueues nothing
  const char* why = attention_refusal(B, T, n_head, head_dim, true);
  if (!why && !(aligned16(qkv) && aligned16(out) && aligned16(lse) && aligned16(dout) && aligned16(dqkv) && aligned16(workspace)))
    why = "pointers must be 16-byte aligned";
  if (!why && workspace_bytes < (size_t)(B * n_head * T) * sizeof(float)) why = "workspace too small";
  if (why) {
    set_error("spq_causal_attention_bwd: %s (B=%lld T=%lld n_head=%lld head_dim=%lld workspace_bytes=%zu)", why, (long long)B,
              (long long)T, (long long)n_head, (long long)head_dim, workspace_bytes);
    return SPQ_ERR_UNSUPPORTED;
  }
  AttBwdArgs g;
  g.qkv = qkv; g.out = out; g.lse = lse; g.dout = dout; g.dqkv = dqkv;
  g.delta = static_cast<const float*>(workspace); g.delta_out = static_cast<float*>(workspace);
  g.T = (int)T; g.H = (int)n_head; g.BH = (int)(B * n_head); g.n_blk = (int)((T + ATT_BLOCK - 1) / ATT_BLOCK);
  g.sqrt_d = (float)sqrt((double)head_dim);
  hipStream_t st = (hipStream_t)stream;
  switch (head_dim) {
    case 16: return launch_attention_bwd<16>(g, st);
    case 32: return launch_attention_bwd<32>(g, st);
    default: return launch_attention_bwd<64>(g, st);
  }
}
