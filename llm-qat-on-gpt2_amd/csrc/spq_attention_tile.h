// The tile plan shared by the causal attention forward (spq_attention.hip) and backward (spq_attention_bwd.hip): one copy of the
// pieces that carry their correctness contracts, all on v_mfma_f32_32x32x2_f32.
//
// A 256-thread workgroup serves one 128-row block of one (sequence, head); wavefront w owns rows 32w .. 32w + 31 of it, one per
// lane & 31, and walks 32-row tiles ANCHORED AT POSITION 0 of the other axis.  A tile goes global -> registers -> LDS in one of
// two images:
//   "rows"  float4 along d -> LDS [row][D + 4].  As the A operand, lane half h reads the D/2 contiguous d of its row with
//           ds_read_b128 (k index of step s = d (D/2)h + s); the B operand is D/2 registers holding the same d of the lane's own
//           row, loaded once per kernel.
//   "cols"  4 consecutive rows of one d -> LDS [d][32 rows + 4], i.e. the tile transposed.
// C/D map of the 32x32 MFMA: lane & 31 = column, register e of lane half h = row 4h + (e & 3) + 8 (e >> 2).  A C/D register set is
// therefore, as it is, the B operand of a product with a "cols" image: step e sums rows 4h + (e & 3) + 8 (e >> 2), h = 0, 1, and
// lane (d, h) reads the A values of steps 4g .. 4g + 3 as ONE ds_read_b128.  Rows at positions >= T are loaded as zeros.
#pragma once
#include "spq_common.h"

namespace spq {

typedef float att_f32x16 __attribute__((ext_vector_type(16)));

constexpr int ATT_BLOCK = 128, ATT_TILE = 32, ATT_TLD = ATT_TILE + 4;

// 1 / sqrt(D) is a power of two for D = 16, 64: scaling q (in dK/dV: k) by it is then the reference's division of the score, bit
// for bit; other head sizes divide the score.  The forward and the backward must agree on this rule: the backward's P is the
// forward's probability only because both compute the score the same way.
constexpr bool att_scale_is_pow2(int D) { return D == 16 || D == 64; }

// what a workgroup and this wavefront of it serve: 128-row block `blk` of (sequence b, head hd).  blockIdx.x = block-major over
// the BH (sequence, head) pairs; `reversed` hands the last block to the first workgroup indices.
struct AttWork {
  int blk, bh, b, hd;
  int64_t C, ld;       // row strides of out / dout [B*T, C] and of qkv / dqkv [B*T, 3C]
  int row0;            // first row of this wavefront; its diagonal tile of the other axis starts there too
  bool active;         // row0 < T (wavefront-uniform)
  int diag;
};
__device__ __forceinline__ AttWork att_work(int n_blk, bool reversed, int BH, int H, int D, int T, int w) {
  AttWork k;
  k.blk = (int)(blockIdx.x / (unsigned)BH);
  if (reversed) k.blk = n_blk - 1 - k.blk;
  k.bh = (int)(blockIdx.x % (unsigned)BH);
  k.b = k.bh / H; k.hd = k.bh % H;
  k.C = (int64_t)H * D; k.ld = 3 * k.C;
  k.row0 = k.blk * ATT_BLOCK + 32 * w;
  k.active = k.row0 < T;
  k.diag = k.row0 / ATT_TILE;
  return k;
}

template <int D>
struct AttRows { static constexpr int N = (ATT_TILE * D / 4 + 255) / 256; float4 r[N]; };
template <int D>
struct AttCols { static constexpr int N = (D * (ATT_TILE / 4) + 255) / 256; float4 r[N]; };

template <int D>
__device__ __forceinline__ void att_load_rows(AttRows<D>& t, const float* __restrict__ base, int64_t ld, int r0, int T, int tid) {
#pragma unroll
  for (int i = 0; i < AttRows<D>::N; ++i) {
    const int idx = tid + 256 * i;
    const int row = idx / (D / 4), c = (idx % (D / 4)) * 4;
    float4 val = make_float4(0.f, 0.f, 0.f, 0.f);
    if (idx < ATT_TILE * D / 4 && r0 + row < T) val = *reinterpret_cast<const float4*>(base + (int64_t)(r0 + row) * ld + c);
    t.r[i] = val;
  }
}

template <int D>
__device__ __forceinline__ void att_store_rows(const AttRows<D>& t, float* __restrict__ s, int tid) {
#pragma unroll
  for (int i = 0; i < AttRows<D>::N; ++i) {
    const int idx = tid + 256 * i;
    if (idx < ATT_TILE * D / 4) *reinterpret_cast<float4*>(s + (idx / (D / 4)) * (D + 4) + (idx % (D / 4)) * 4) = t.r[i];
  }
}

template <int D>
__device__ __forceinline__ void att_load_cols(AttCols<D>& t, const float* __restrict__ base, int64_t ld, int r0, int T, int tid) {
#pragma unroll
  for (int i = 0; i < AttCols<D>::N; ++i) {
    const int idx = tid + 256 * i;
    const int d = idx % D, row = r0 + (idx / D) * 4;
    float4 val = make_float4(0.f, 0.f, 0.f, 0.f);
    if (idx < D * (ATT_TILE / 4)) {
      const float* p = base + (int64_t)row * ld + d;
      if (row + 0 < T) val.x = p[0];
      if (row + 1 < T) val.y = p[ld];
      if (row + 2 < T) val.z = p[2 * ld];
      if (row + 3 < T) val.w = p[3 * ld];
    }
    t.r[i] = val;
  }
}

// (LDS rows >= D of an image of (D + 31) / 32 blocks of 32 -- D = 16, 80 -- are never written: they feed only the accumulator rows
// >= D, which att_store_acc never stores)
template <int D>
__device__ __forceinline__ void att_store_cols(const AttCols<D>& t, float* __restrict__ s, int tid) {
#pragma unroll
  for (int i = 0; i < AttCols<D>::N; ++i) {
    const int idx = tid + 256 * i;
    if (idx < D * (ATT_TILE / 4)) *reinterpret_cast<float4*>(s + (idx % D) * ATT_TLD + (idx / D) * 4) = t.r[i];
  }
}

__device__ __forceinline__ void att_zero(att_f32x16& c) {
#pragma unroll
  for (int e = 0; e < 16; ++e) c[e] = 0.f;
}
template <int N>
__device__ __forceinline__ void att_zero(att_f32x16 (&acc)[N]) {
#pragma unroll
  for (int i = 0; i < N; ++i) att_zero(acc[i]);
}

// D/2 floats of one row into registers, times `scale`
template <int D>
__device__ __forceinline__ void att_load_half_row(float (&r)[D / 2], const float* __restrict__ p, float scale) {
#pragma unroll
  for (int i = 0; i < D / 8; ++i) {
    const float4 v4 = *reinterpret_cast<const float4*>(p + 4 * i);
    r[4 * i + 0] = v4.x * scale; r[4 * i + 1] = v4.y * scale; r[4 * i + 2] = v4.z * scale; r[4 * i + 3] = v4.w * scale;
  }
}

// C = A . B with A = a "rows" image (ap = this lane's row + (D/2) h), B = the registers of att_load_half_row: S^T = K . Q^T
template <int D>
__device__ __forceinline__ att_f32x16 att_rows_times_regs(const float* __restrict__ ap, const float (&b)[D / 2]) {
  att_f32x16 c;
  att_zero(c);
#pragma unroll
  for (int i = 0; i < D / 8; ++i) {
    const float4 a = *reinterpret_cast<const float4*>(ap + 4 * i);
    c = __builtin_amdgcn_mfma_f32_32x32x2f32(a.x, b[4 * i + 0], c, 0, 0, 0);
    c = __builtin_amdgcn_mfma_f32_32x32x2f32(a.y, b[4 * i + 1], c, 0, 0, 0);
    c = __builtin_amdgcn_mfma_f32_32x32x2f32(a.z, b[4 * i + 2], c, 0, 0, 0);
    c = __builtin_amdgcn_mfma_f32_32x32x2f32(a.w, b[4 * i + 3], c, 0, 0, 0);
  }
  return c;
}

// acc[d block] += A . B with A = a "cols" image (ap = row (lane & 31) of it + 4h), B = a C/D register set as it was born:
// O^T += V^T . P^T
template <int NDB>
__device__ __forceinline__ void att_cols_times_cd(att_f32x16 (&acc)[NDB], const float* __restrict__ ap, const att_f32x16& b) {
#pragma unroll
  for (int gi = 0; gi < 4; ++gi) {
#pragma unroll
    for (int i = 0; i < NDB; ++i) {
      const float4 a = *reinterpret_cast<const float4*>(ap + i * 32 * ATT_TLD + 8 * gi);
      acc[i] = __builtin_amdgcn_mfma_f32_32x32x2f32(a.x, b[4 * gi + 0], acc[i], 0, 0, 0);
      acc[i] = __builtin_amdgcn_mfma_f32_32x32x2f32(a.y, b[4 * gi + 1], acc[i], 0, 0, 0);
      acc[i] = __builtin_amdgcn_mfma_f32_32x32x2f32(a.z, b[4 * gi + 2], acc[i], 0, 0, 0);
      acc[i] = __builtin_amdgcn_mfma_f32_32x32x2f32(a.w, b[4 * gi + 3], acc[i], 0, 0, 0);
    }
  }
}

// the accumulator blocks (rows = d, through the C/D map) -> D floats of this lane's row at op, each times `mul` (MUL) or over `div`
template <int D, int NDB, bool MUL>
__device__ __forceinline__ void att_store_acc(const att_f32x16 (&acc)[NDB], float* __restrict__ op, int h, float mul, float div) {
#pragma unroll
  for (int i = 0; i < NDB; ++i) {
#pragma unroll
    for (int gi = 0; gi < 4; ++gi) {
      const int dd = i * 32 + 8 * gi + 4 * h;    // rows 4h + (e & 3) + 8 (e >> 2) of block i, e = 4 gi .. 4 gi + 3
      if (dd < D) {
        float4 v4;
        if (MUL) v4 = make_float4(acc[i][4 * gi + 0] * mul, acc[i][4 * gi + 1] * mul, acc[i][4 * gi + 2] * mul, acc[i][4 * gi + 3] * mul);
        else v4 = make_float4(acc[i][4 * gi + 0] / div, acc[i][4 * gi + 1] / div, acc[i][4 * gi + 2] / div, acc[i][4 * gi + 3] / div);
        *reinterpret_cast<float4*>(op + dd) = v4;
      }
    }
  }
}

}  // namespace spq
