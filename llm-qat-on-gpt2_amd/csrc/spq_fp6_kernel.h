// SPQ_PATH_FP6: the dense contraction on v_mfma_scale_f32_16x16x128_f8f6f4 with FP6 (e2m3) operands.
//
// Valid for a symmetric min-max input quantizer of 2..4 bits: the integer levels |q| <= 7 are exact e2m3 numbers.  The weight operand
//        W'[n,k] = FQ(W)[n,k] * sx[k]                 (exact product, fp64)
// is scaled per output row by a power of two 2^E[n] that puts the row maximum into [2^23, 2^24), rounded ONCE to the integer
// w = rint(W' 2^E[n]) (fp64, ties to even) and written as five balanced radix-32 digits, w = sum_i d_i 32^i, |d_i| <= 16, each stored as
// the e2m3 code of d_i / 8 (e2m3 holds every multiple of 1/8 up to 2); the digit weight 8 * 32^i is the instruction's block scale:
//        y[m,n] = 2^-E[n] sum_i 2^(3 + 5 i) sum_k q[m,k] (d_i[n,k] / 8)  + bias[n]        five MFMAs per 128-deep k block and 16 x 16 outputs
// Every product and every partial sum below 2^24 is exact; the fp32 accumulation of the MFMA is the only rounding.
//
// Packed plane layout (activation levels and each digit plane): rows in pairs of 32, k in blocks of 128 (k padded with zero codes);
// one (pair, k block) = 3072 B = [rec0 16-B parts 1 KB | rec1 16-B parts 1 KB | rec0 8-B parts 512 B | rec1 8-B parts 512 B], rec = 16 rows;
// lane l = (row & 15) + 16 (k / 32 % 4) owns a 24-B field = its row's 32 codes of k = 32 (l >> 4) .. + 31, 6 bits each, LSB first:
// bytes 0..15 in the 16-B part, bytes 16..23 in the 8-B part.  Block (pair p, k block kb) of a plane with KB k blocks starts at
// (p * KB + kb) * 3072.  tests/fp6_ref.py is the numpy reference of this layout.
//
// Included by spq_f16x2.hip (it uses that file's activation-pass arguments, LoRA stage layout and epilogue helpers).
#pragma once
// (included inside namespace spq)

constexpr int F6_REC = 1536;                        // one MFMA operand tile: 16 rows x 128 k x 6 bit
constexpr int F6_PAIR = 2 * F6_REC;                 // two records interleaved (32 rows x 128 k)
constexpr int F6_PLANE = 4 * F6_PAIR;               // 128 rows x 128 k of one operand plane: 12 KB
constexpr int F6_NL = 5;                            // weight digits
constexpr int F6_HALF = 3 * F6_PLANE;               // a half stage: 36 KB
constexpr int F6_LDS = 3 * 16384;                   // the LoRA-up stage [t 16 KB | B-hi 16 KB | B-lo 16 KB] is the larger tenant: 48 KB, three workgroups per CU

// w_prep of SPQ_PATH_FP6: [five digit planes, each (Np / 32) * KB * 3072 B][Bhi Np x Rp fp16][Blo][bfac Np floats], Np = ceil(N/128)*128,
// KB = ceil(K/128), Rp = ceil(r/64)*64.  bfac[n] = 2^(E[n] - eb[n]) brings the LoRA partial sums (B limbs carry 2^eb[n]) to the digit sum's units.
struct PrepLayoutFp6 { int64_t Np, KB, Rp; size_t plane, off_bhi, off_blo, off_bfac, total; };
static PrepLayoutFp6 make_prep_layout_fp6(int64_t N, int64_t K, int64_t r) {
  PrepLayoutFp6 L;
  L.Np = pad_to(N, 128); L.KB = (K + 127) / 128; L.Rp = r > 0 ? pad_to(r, 64) : 0;
  L.plane = (size_t)(L.Np / 32) * L.KB * F6_PAIR;
  size_t o = (size_t)F6_NL * L.plane;
  L.off_bhi = o; o += pad_to((size_t)L.Np * L.Rp * 2, 256);
  L.off_blo = o; o += pad_to((size_t)L.Np * L.Rp * 2, 256);
  L.off_bfac = o; o += pad_to((size_t)L.Np * 4, 256);
  L.total = o + 256;
  return L;
}

__device__ __forceinline__ unsigned e2m3_of_eighths(int d) {          // the code of d / 8, |d| <= 16
  const int a = d < 0 ? -d : d;
  const unsigned code = a < 8 ? (unsigned)a : (a < 16 ? (0x08u | (unsigned)(a - 8)) : 0x10u);
  return (d < 0 ? 0x20u : 0u) | code;
}
__device__ __forceinline__ unsigned e2m3_of_level(float q) {          // integer level |q| <= 7: 0x1E1C1A1814100800 holds the eight codes
  const int qi = (int)q, a = qi < 0 ? -qi : qi;
  const unsigned code = (unsigned)((0x1E1C1A1814100800ull >> (8 * a)) & 0x3F);
  return (qi < 0 ? 0x20u : 0u) | code;
}

// Activation store of the FP6 form.  The 16 lanes of a row hold four consecutive levels each of one 64-column chunk `c`: the lane
// at chunk position j (0..15; its lane index within the row's 16 is j ^ xr) has columns 4j .. 4j + 3 as the 24-bit value c24.  The
// row's two 24-B fields (k quarters 2 (c & 1) and + 1) are assembled with eight shuffles; the lanes at positions 0 / 8 store the
// 16-B parts and those at 1 / 9 the 8-B parts: exactly two store instructions per wave and chunk.  m < M (callers clamp).
__device__ __forceinline__ void fp6_store_chunk(unsigned char* A6, int KB, int m, int c, int xr, unsigned c24, int lane) {
  const int j = (lane & 15) ^ xr, f = j >> 3, jj = j & 7;
  unsigned s[8];
#pragma unroll
  for (int i = 0; i < 8; ++i) s[i] = (unsigned)__shfl((int)c24, (lane & 48) | ((8 * f + i) ^ xr), 64);
  unsigned char* base = A6 + ((int64_t)(m >> 5) * KB + (c >> 1)) * F6_PAIR;
  const int rec = (m >> 4) & 1, L = (m & 15) + 16 * (2 * (c & 1) + f);
  if (jj == 0)
    *reinterpret_cast<uint4*>(base + rec * 1024 + L * 16) =
        make_uint4(s[0] | (s[1] << 24), (s[1] >> 8) | (s[2] << 16), (s[2] >> 16) | (s[3] << 8), s[4] | (s[5] << 24));
  if (jj == 1)
    *reinterpret_cast<uint2*>(base + 2048 + rec * 512 + L * 8) = make_uint2((s[5] >> 8) | (s[6] << 16), (s[6] >> 16) | (s[7] << 8));
}
__device__ __forceinline__ unsigned fp6_code4(float q0, float q1, float q2, float q3) {
  return e2m3_of_level(q0) | (e2m3_of_level(q1) << 6) | (e2m3_of_level(q2) << 12) | (e2m3_of_level(q3) << 18);
}

// =================================================================================================
// Weight preparation: one workgroup per pair of 32 output rows.  Pass 1: row maximum of |W'| (fp64) -> E[n], rowscale[n] = 2^-E[n], and
// the LoRA-B limbs with their own exponent.  Pass 2: per 128-deep k block the five digit codes of w = rint(W' 2^E) through LDS into
// the packed planes.  FQ(W) is recomputed in pass 2 (the rows are L2-resident).
// =================================================================================================
struct PrepFp6Args { unsigned char* planes; int64_t plane_stride; int KB; float* bfac; };

__global__ __launch_bounds__(256) void prep_fp6_kernel(PrepArgs a, PrepFp6Args f) {
  if ((int)blockIdx.x >= a.row_blocks) { fq_transpose_tile(a, blockIdx.x - a.row_blocks); return; }
  __shared__ unsigned char codes[F6_NL][32][128];
  const int tid = threadIdx.x, row = tid >> 3, sub = tid & 7;
  const int pair = blockIdx.x, n = pair * 32 + row;
  const bool live = n < a.N;
  const float swn = live ? a.sw[a.w_pc ? n : 0] : 1.f, zwn = live ? a.zw[a.w_pc ? n : 0] : 0.f;
  double mx = 0.0;
  int bad = 0;                                            // a NaN / Inf element of W' (fmax would drop a NaN)
  if (live)
    for (int k = sub; k < a.K; k += 8) {
      const float wq = fq_dispatch(a.W[(int64_t)n * a.K + k], swn, zwn, a.w_bits, a.w_qtype, a.w_sym);
      const double wa = fabs((double)wq * (double)a.sx[a.x_pc ? k : 0]);
      if (!(wa < (double)INFINITY)) bad = 1; else mx = fmax(mx, wa);
    }
  mx = fmax(mx, __shfl_xor(mx, 1, 64)); mx = fmax(mx, __shfl_xor(mx, 2, 64)); mx = fmax(mx, __shfl_xor(mx, 4, 64));
  bad |= __shfl_xor(bad, 1, 64); bad |= __shfl_xor(bad, 2, 64); bad |= __shfl_xor(bad, 4, 64);
  int E = 0;
  if (mx > 0.0) { int ex; (void)frexp(mx, &ex); E = 24 - ex; }   // mx 2^E in [2^23, 2^24)
  // rowscale = 2^-E must be a normal float.  A row too small for that (max < 2^-102) keeps E = 126 and loses low digits only; a row
  // too large (max >= 2^150) or with a non-finite element has no digit form: its rowscale is NaN, so its output column is NaN
  // for every token (the f16 paths give NaN / Inf there too) instead of silently finite.
  if (E < -126) bad = 1;
  E = min(max(E, -126), 126);
  if (sub == 0) a.rowscale[n] = bad ? __builtin_nanf("") : ldexpf(1.f, -E);
  // LoRA-B column n: B' = scaling * FQ(B)[:, n], two fp16 limbs of B' 2^eb[n]
  if (a.Bhi) {
    const float sbn = (live && a.B) ? a.sb[a.b_pc ? n : 0] : 1.f, zbn = (live && a.B) ? a.zb[a.b_pc ? n : 0] : 0.f;
    float bmax = 0.f;
    if (live && a.B)
      for (int j = sub; j < a.r; j += 8)
        bmax = fmaxf(bmax, fabsf(fq_dispatch(a.B[(int64_t)j * a.N + n], sbn, zbn, a.b_bits, a.b_qtype, a.b_sym) * a.scaling));
    bmax = fmaxf(bmax, __shfl_xor(bmax, 1, 64)); bmax = fmaxf(bmax, __shfl_xor(bmax, 2, 64)); bmax = fmaxf(bmax, __shfl_xor(bmax, 4, 64));
    const float pb = pow2_scale_for(bmax);
    for (int j = sub; j < a.Rp; j += 8) {
      _Float16 h = (_Float16)0.f, l = (_Float16)0.f;
      if (live && a.B && j < a.r) split2((fq_dispatch(a.B[(int64_t)j * a.N + n], sbn, zbn, a.b_bits, a.b_qtype, a.b_sym) * a.scaling) * pb, h, l);
      a.Bhi[(int64_t)n * a.Rp + j] = h; a.Blo[(int64_t)n * a.Rp + j] = l;
    }
    if (sub == 0) { int eb; (void)frexpf(pb, &eb); f.bfac[n] = ldexpf(1.f, min(max(E - (eb - 1), -126), 126)); }
  } else if (sub == 0) f.bfac[n] = 1.f;
  __syncthreads();
  const int k0 = sub * 16;
  for (int kb = 0; kb < f.KB; ++kb) {
#pragma unroll 4
    for (int i = 0; i < 16; ++i) {
      const int k = kb * 128 + k0 + i;
      long long wi = 0;
      if (live && k < a.K) {
        const float wq = fq_dispatch(a.W[(int64_t)n * a.K + k], swn, zwn, a.w_bits, a.w_qtype, a.w_sym);
        const double ws = rint(ldexp((double)wq * (double)a.sx[a.x_pc ? k : 0], E));       // the ONE rounding, ties to even
        wi = (fabs(ws) <= 16777216.0) ? (long long)ws : 0;                                     // (a non-finite weight: no digits)
      }
      const int sgn = wi < 0 ? -1 : 1;
      int wa = (int)(wi < 0 ? -wi : wi);
#pragma unroll
      for (int pl = 0; pl < F6_NL; ++pl) {
        int d = wa & 31; if (d > 16) d -= 32;
        wa = (wa - d) >> 5;
        codes[pl][row][k0 + i] = (unsigned char)e2m3_of_eighths(sgn * d);
      }
    }
    __syncthreads();
    if (tid < 128) {                       // thread t owns the field of row (t & 15) + 16 (t >> 6), k quarter (t >> 4) & 3
      const int l15 = tid & 15, kq = (tid >> 4) & 3, rec = tid >> 6, frow = rec * 16 + l15, lane = l15 + 16 * kq;
#pragma unroll
      for (int pl = 0; pl < F6_NL; ++pl) {
        unsigned w6[6] = {0, 0, 0, 0, 0, 0};
#pragma unroll
        for (int i = 0; i < 32; ++i) {
          const unsigned cd = codes[pl][frow][32 * kq + i];
          const int bit = 6 * i;
          w6[bit >> 5] |= cd << (bit & 31);
          if ((bit & 31) > 26) w6[(bit >> 5) + 1] |= cd >> (32 - (bit & 31));
        }
        unsigned char* base = f.planes + (int64_t)pl * f.plane_stride + ((int64_t)pair * f.KB + kb) * F6_PAIR;
        *reinterpret_cast<uint4*>(base + rec * 1024 + lane * 16) = make_uint4(w6[0], w6[1], w6[2], w6[3]);
        *reinterpret_cast<uint2*>(base + 2048 + rec * 512 + lane * 8) = make_uint2(w6[4], w6[5]);
      }
    }
    __syncthreads();
  }
}

