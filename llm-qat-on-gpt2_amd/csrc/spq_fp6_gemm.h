// SPQ_PATH_FP6, the contraction kernel (format and packing: spq_fp6_kernel.h).  Included by spq_f16x2.hip after the f16 contraction
// kernel, whose LoRA stage layout (swz), epilogue slices (EPI_WAVE) and tile order (T128_GROUP_M) it shares.
#pragma once
// (included inside namespace spq)

// =================================================================================================
// The contraction: 128 x 128 tiles, 4 waves (2 x 2 of 64 x 64 outputs), ONE buffer through which the half stages X = {A, planes 0, 1}
// and Y = {planes 2, 3, 4} of every k block pass in turn (wait + barrier, multiply, barrier, issue the next half), the A fragments kept
// in registers from X to Y; three workgroups per CU.  The LoRA-up stages (fp16 limbs, 64-deep, v_mfma_f32_16x16x32_f16 into the same
// accumulators) run first; their partial sums are brought to the digit sum's units by rowinv[m] * bfac[n] (powers of two: exact).
// No wave waits on another except at workgroup barriers.
// =================================================================================================
struct GemmFp6Args {
  const unsigned char* A6;      // [Mp/32 pairs][KB][3072 B]
  const unsigned char* W6;      // [5][Np/32 pairs][KB][3072 B]
  int64_t plane_stride;
  const float *rowscale, *bfac, *bias;   // [Np], [Np], [N] (nullable)
  float* y;
  int M, N, KB;
  int tiles_m, tiles_n;         // 128 x 128 tiles
  const _Float16 *thi, *tlo, *Bhi, *Blo; const float* rowinv; int Rp;   // Rp = 0: no LoRA-up stages
};

template <int EPI, bool RAG>    // EPI 1: gelu(y); RAG: N % 4 != 0 (rows of y not 16-B aligned: element stores)
__global__ __launch_bounds__(256, 3) void gemm_fp6_kernel(GemmFp6Args g) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int tid = threadIdx.x, lane = tid & 63;
  const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wm = w >> 1, wn = w & 1;
  const int l15 = lane & 15, q4 = lane >> 4;
  const int nwg = g.tiles_m * g.tiles_n;
  const int KB = g.KB;
  const int gstride = (int)gridDim.x;
  auto tile_of = [&](int p, int& bm, int& bn) {              // the f16 kernel's XCD-aware band order
    const int q8 = nwg >> 3, r8 = nwg & 7, xcd = p & 7;
    const int wgid = (xcd < r8 ? xcd * (q8 + 1) : r8 * (q8 + 1) + (xcd - r8) * q8) + (p >> 3);
    constexpr int GROUP_M = T128_GROUP_M;
    const int band = wgid / (GROUP_M * g.tiles_n);
    const int band_rows = min(GROUP_M, g.tiles_m - band * GROUP_M);
    const int in_band = wgid - band * GROUP_M * g.tiles_n;
    bm = (band * GROUP_M + in_band % band_rows) * 128;
    bn = (in_band / band_rows) * 128;
  };
  int p = blockIdx.x;
  if (p >= nwg) return;
  int bm, bn;
  tile_of(p, bm, bn);
  const unsigned lds0 = (unsigned)(uintptr_t)(__attribute__((address_space(3))) char*)smem;
  const unsigned voff = (unsigned)lane * 16u;
  auto glds = [&](const unsigned char* sbase, unsigned lds_addr) {
    {   // (wave-uniform by construction; say so to the compiler: the "s" constraint needs scalar registers)
      const unsigned long long a64 = (unsigned long long)sbase;
      const unsigned lo = __builtin_amdgcn_readfirstlane((unsigned)a64), hi = __builtin_amdgcn_readfirstlane((unsigned)(a64 >> 32));
      sbase = (const unsigned char*)(((unsigned long long)hi << 32) | lo);
      lds_addr = __builtin_amdgcn_readfirstlane(lds_addr);
    }
    asm volatile("s_mov_b32 m0, %2\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %0, %1" :: "v"(voff), "s"(sbase), "s"(lds_addr) : "memory", "m0");
  };
  // a half stage = three 12-KB planes = 36 pieces of 1 KB; wave w copies the three pieces of pair w of each plane.  Six running source pointers
  // (A and the five planes, pair w of the current tile), + 3 KB per k block.
  const unsigned char* src6[6];
  auto set_tile = [&](int tbm, int tbn) {
    src6[0] = g.A6 + ((int64_t)(tbm / 32 + w) * KB) * F6_PAIR;
#pragma unroll
    for (int pl = 0; pl < 5; ++pl) src6[1 + pl] = g.W6 + (int64_t)pl * g.plane_stride + ((int64_t)(tbn / 32 + w) * KB) * F6_PAIR;
  };
  auto issue_x = [&]() {                                       // half X of the NEXT k block of the running pointers: A, planes 0, 1
#pragma unroll
    for (int j = 0; j < 3; ++j) { const unsigned dst = lds0 + (unsigned)(j * F6_PLANE + 3 * w * 1024); glds(src6[j], dst); glds(src6[j] + 1024, dst + 1024u); glds(src6[j] + 2048, dst + 2048u); }
  };
  auto issue_y = [&]() {                                       // half Y of the same k block: planes 2, 3, 4; then the pointers advance
#pragma unroll
    for (int j = 0; j < 3; ++j) { const unsigned dst = lds0 + (unsigned)(j * F6_PLANE + 3 * w * 1024); glds(src6[3 + j], dst); glds(src6[3 + j] + 1024, dst + 1024u); glds(src6[3 + j] + 2048, dst + 2048u); }
#pragma unroll
    for (int j = 0; j < 6; ++j) src6[j] += F6_PAIR;
  };
  // ---- hand-allocated fragment registers: one asm block per plane.  v[120:143] and v[144:167] hold the four 6-register weight operands of a
  // plane (two fixed sets, declared clobbered in every block, so the compiler keeps out of them and their contents survive from block to block);
  // a plane's eight reads are issued one plane ahead of its sixteen MFMAs; the sixteen accumulators are tied operands, the four activation
  // operands inputs.
  // The contents of v[120:167] live from an rd() block to the mm() block that consumes them only because every asm statement between
  // them names the registers as clobbered and nothing else sits between them but waits and barriers: checked in the disassembly of
  // the three instantiations (no compiler-generated instruction and no scratch access touches v120..v167 inside the k loop; the
  // kernel's spills, 17-26 VGPRs, are all around the LoRA stages and the epilogue).  Re-check after any change to this loop.
  typedef int v6i __attribute__((ext_vector_type(6)));
  v6i fa[4];
  f32x4 acc[4][4];
  const unsigned a16_0 = lds0 + (unsigned)(2 * wn * F6_PAIR + lane * 16), a8_0 = lds0 + (unsigned)(2 * wn * F6_PAIR + 2048 + lane * 8);
  const int scale_a = 127;
#define F6_MFMA(tm, tn, breg) "v_mfma_scale_f32_16x16x128_f8f6f4 %[c" #tm #tn "], %[a" #tm "], " breg ", %[c" #tm #tn "], %[sa], %[sb] op_sel_hi:[0,0,0] cbsz:2 blgp:2\n\t"
#define F6_ROW0(tm) F6_MFMA(tm, 0, "v[120:125]") F6_MFMA(tm, 1, "v[126:131]") F6_MFMA(tm, 2, "v[132:137]") F6_MFMA(tm, 3, "v[138:143]")
#define F6_ROW1(tm) F6_MFMA(tm, 0, "v[144:149]") F6_MFMA(tm, 1, "v[150:155]") F6_MFMA(tm, 2, "v[156:161]") F6_MFMA(tm, 3, "v[162:167]")
#define F6_CLOB0 "v120", "v121", "v122", "v123", "v124", "v125", "v126", "v127", "v128", "v129", "v130", "v131", "v132", "v133", "v134", "v135", "v136", "v137", "v138", "v139", "v140", "v141", "v142", "v143"
#define F6_CLOB1 "v144", "v145", "v146", "v147", "v148", "v149", "v150", "v151", "v152", "v153", "v154", "v155", "v156", "v157", "v158", "v159", "v160", "v161", "v162", "v163", "v164", "v165", "v166", "v167"
  auto rd = [&](int set, int off) {
    const unsigned a16 = a16_0 + (unsigned)off, a8 = a8_0 + (unsigned)off;
    if (set == 0)
      asm volatile("ds_read_b128 v[120:123], %[p16]\n\tds_read_b64 v[124:125], %[p8]\n\tds_read_b128 v[126:129], %[p16] offset:1024\n\tds_read_b64 v[130:131], %[p8] offset:512\n\t"
                   "ds_read_b128 v[132:135], %[p16] offset:3072\n\tds_read_b64 v[136:137], %[p8] offset:3072\n\tds_read_b128 v[138:141], %[p16] offset:4096\n\tds_read_b64 v[142:143], %[p8] offset:3584"
                   :: [p16] "v"(a16), [p8] "v"(a8) : "memory", F6_CLOB0, F6_CLOB1);
    else
      asm volatile("ds_read_b128 v[144:147], %[p16]\n\tds_read_b64 v[148:149], %[p8]\n\tds_read_b128 v[150:153], %[p16] offset:1024\n\tds_read_b64 v[154:155], %[p8] offset:512\n\t"
                   "ds_read_b128 v[156:159], %[p16] offset:3072\n\tds_read_b64 v[160:161], %[p8] offset:3072\n\tds_read_b128 v[162:165], %[p16] offset:4096\n\tds_read_b64 v[166:167], %[p8] offset:3584"
                   :: [p16] "v"(a16), [p8] "v"(a8) : "memory", F6_CLOB0, F6_CLOB1);
  };
#define F6_MM(ROWS, WAIT) asm volatile("s_waitcnt lgkmcnt(" #WAIT ")\n\t" ROWS(0) ROWS(1) ROWS(2) ROWS(3) \
        : [c00] "+v"(acc[0][0]), [c01] "+v"(acc[0][1]), [c02] "+v"(acc[0][2]), [c03] "+v"(acc[0][3]), [c10] "+v"(acc[1][0]), [c11] "+v"(acc[1][1]), [c12] "+v"(acc[1][2]), [c13] "+v"(acc[1][3]), \
          [c20] "+v"(acc[2][0]), [c21] "+v"(acc[2][1]), [c22] "+v"(acc[2][2]), [c23] "+v"(acc[2][3]), [c30] "+v"(acc[3][0]), [c31] "+v"(acc[3][1]), [c32] "+v"(acc[3][2]), [c33] "+v"(acc[3][3]) \
        : [a0] "v"(fa[0]), [a1] "v"(fa[1]), [a2] "v"(fa[2]), [a3] "v"(fa[3]), [sa] "v"(scale_a), [sb] "v"(sb) : "memory", F6_CLOB0, F6_CLOB1)
  auto mm = [&](int set, int pl, bool more_in_flight) {        // more_in_flight: the OTHER set's eight reads were issued after this set's
    const int sb = 127 + 3 + 5 * pl;                           // E8M0: the digit's weight 8 * 32^pl
    if (set == 0) { if (more_in_flight) F6_MM(F6_ROW0, 8); else F6_MM(F6_ROW0, 0); }
    else { if (more_in_flight) F6_MM(F6_ROW1, 8); else F6_MM(F6_ROW1, 0); }
  };
  auto load_a = [&]() {                                        // the activation operands of the wave's four row tiles (plane 0 of the X half)
#pragma unroll
    for (int t = 0; t < 4; ++t) {
      const int r = 4 * wm + t;
      const char* pb = smem + (r >> 1) * F6_PAIR;
      const uint4 a = *reinterpret_cast<const uint4*>(pb + (r & 1) * 1024 + lane * 16);
      const uint2 b2 = *reinterpret_cast<const uint2*>(pb + 2048 + (r & 1) * 512 + lane * 8);
      fa[t][0] = (int)a.x; fa[t][1] = (int)a.y; fa[t][2] = (int)a.z; fa[t][3] = (int)a.w; fa[t][4] = (int)b2.x; fa[t][5] = (int)b2.y;
    }
  };
  // ---- LoRA-up stages: the f16 kernel's (fp16 limbs, 64-deep, [t 16 KB | B-hi 16 KB | B-lo 16 KB] with its XOR swizzle)
  const int nlb = g.Rp / 64;
  const int prow8 = lane >> 3, pchunk = lane & 7;
  auto issue_lora = [&](int j, int which, int tbm, int tbn) {
    const _Float16* A = (which ? g.tlo : g.thi) + (int64_t)tbm * g.Rp + j * 64;
    const _Float16* Bh = g.Bhi + (int64_t)tbn * g.Rp + j * 64;
    const _Float16* Bl = g.Blo + (int64_t)tbn * g.Rp + j * 64;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int row = (4 * w + i) * 8 + prow8, col = swz(row, pchunk) * 8;
      glds16(A + (row * g.Rp + col), smem + (4 * w + i) * 1024);
      if (!which) { glds16(Bh + (row * g.Rp + col), smem + 16384 + (4 * w + i) * 1024); glds16(Bl + (row * g.Rp + col), smem + 32768 + (4 * w + i) * 1024); }
    }
  };
  auto lora_stage = [&](bool two) {                          // one operand set live at a time
    const int sx7 = (l15 >> 1) & 7;
#pragma unroll
    for (int s2 = 0; s2 < 2; ++s2) {
      const int koff = ((4 * s2 + q4) ^ sx7) * 16;
      f16x8 a[4], bb[4];
#pragma unroll
      for (int t = 0; t < 4; ++t) {
        a[t] = *reinterpret_cast<const f16x8*>(smem + (wm * 64 + l15) * 128 + t * 2048 + koff);
        bb[t] = *reinterpret_cast<const f16x8*>(smem + 16384 + (wn * 64 + l15) * 128 + t * 2048 + koff);
      }
#pragma unroll
      for (int tm = 0; tm < 4; ++tm)
#pragma unroll
        for (int tn = 0; tn < 4; ++tn) acc[tm][tn] = __builtin_amdgcn_mfma_f32_16x16x32_f16(a[tm], bb[tn], acc[tm][tn], 0, 0, 0);
      __builtin_amdgcn_sched_barrier(0);
      if (two) {
#pragma unroll
        for (int t = 0; t < 4; ++t) bb[t] = *reinterpret_cast<const f16x8*>(smem + 32768 + (wn * 64 + l15) * 128 + t * 2048 + koff);
#pragma unroll
        for (int tm = 0; tm < 4; ++tm)
#pragma unroll
          for (int tn = 0; tn < 4; ++tn) acc[tm][tn] = __builtin_amdgcn_mfma_f32_16x16x32_f16(a[tm], bb[tn], acc[tm][tn], 0, 0, 0);
        __builtin_amdgcn_sched_barrier(0);
      }
    }
  };
  set_tile(bm, bn);
  if (nlb > 0) issue_lora(0, 0, bm, bn); else issue_x();
  int prio_ctr = (int)(blockIdx.x / (gridDim.x / 3 > 0 ? gridDim.x / 3 : 1));
  int stage_ctr = 0;
  while (true) {
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
      for (int j = 0; j < 4; ++j)
#pragma unroll
        for (int e = 0; e < 4; ++e) acc[i][j][e] = 0.f;
    const int pn = p + gstride;
    const bool more = pn < nwg;
    int nbm = 0, nbn = 0;
    if (more) tile_of(pn, nbm, nbn);
#pragma unroll 1
    for (int j = 0; j < nlb; ++j) {
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); __syncthreads();
      lora_stage(true);                                      // thi x {Bhi, Blo}
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory"); __builtin_amdgcn_s_barrier(); asm volatile("" ::: "memory");
      issue_lora(j, 1, bm, bn);                              // tlo; its B-hi is still in the buffer
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); __syncthreads();
      lora_stage(false);                                     // tlo x Bhi
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory"); __builtin_amdgcn_s_barrier(); asm volatile("" ::: "memory");
      if (j + 1 < nlb) issue_lora(j + 1, 0, bm, bn); else issue_x();
    }
    if (nlb > 0) {                                           // LoRA partial sums (units 2^eb[n] 2^g[m]) -> units of the digit sum 2^E[n]
      float bf[4];
#pragma unroll
      for (int tn = 0; tn < 4; ++tn) bf[tn] = g.bfac[bn + wn * 64 + tn * 16 + l15];
#pragma unroll
      for (int tm = 0; tm < 4; ++tm) {
        const f32x4 riv = *reinterpret_cast<const f32x4*>(g.rowinv + bm + wm * 64 + tm * 16 + 4 * q4);
#pragma unroll
        for (int e = 0; e < 4; ++e)
#pragma unroll
          for (int tn = 0; tn < 4; ++tn) acc[tm][tn][e] = (acc[tm][tn][e] * riv[e]) * bf[tn];
      }
    }
#pragma unroll 1
    for (int kb = 0; kb < KB; ++kb) {
      {                                                      // the CU's three workgroups take the issue priorities in turn (as the f16 kernel)
        const int per = max(1, (KB * ((nwg + gstride - 1) / gstride) + 5) / 6);
        if (stage_ctr % per == 0) { const int pr = (prio_ctr + stage_ctr / per) % 3; if (pr == 0) __builtin_amdgcn_s_setprio(0); else if (pr == 1) __builtin_amdgcn_s_setprio(1); else __builtin_amdgcn_s_setprio(2); }
        ++stage_ctr;
      }
      const bool last = kb + 1 == KB;
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");         // X(kb) has landed
      __builtin_amdgcn_s_barrier(); asm volatile("" ::: "memory");
      load_a();
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");        // (the activation operands: compiler-managed reads; the counted waits below start from zero)
      rd(0, F6_PLANE); rd(1, 2 * F6_PLANE); mm(0, 0, true); mm(1, 1, false);
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
      __builtin_amdgcn_s_barrier(); asm volatile("" ::: "memory");   // every wave is done with X
      issue_y();
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");         // Y(kb) has landed
      __builtin_amdgcn_s_barrier(); asm volatile("" ::: "memory");
      rd(0, 0); rd(1, F6_PLANE); mm(0, 2, true); rd(0, 2 * F6_PLANE); mm(1, 3, true); mm(0, 4, false);
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
      __builtin_amdgcn_s_barrier(); asm volatile("" ::: "memory");   // every wave is done with Y
      if (!last) issue_x();
    }
    // the f16 kernel's epilogue: scale, bias, transpose through per-wave LDS slices (inside the free stage buffer), whole 128-B lines
    float4 ep_rs[2], ep_bv[2];
#pragma unroll
    for (int tn = 0; tn < 2; ++tn) {
      const int n = bn + wn * 64 + tn * 32 + (lane & 7) * 4;
      ep_rs[tn] = make_float4(0.f, 0.f, 0.f, 0.f); ep_bv[tn] = ep_rs[tn];
      if (n < g.N) {
        ep_rs[tn] = *reinterpret_cast<const float4*>(g.rowscale + n);     // [Np]: padded
        if (g.bias) {
          if (!RAG) ep_bv[tn] = *reinterpret_cast<const float4*>(g.bias + n);
          else {
            ep_bv[tn].x = g.bias[n];
            if (n + 1 < g.N) ep_bv[tn].y = g.bias[n + 1];
            if (n + 2 < g.N) ep_bv[tn].z = g.bias[n + 2];
            if (n + 3 < g.N) ep_bv[tn].w = g.bias[n + 3];
          }
        }
      }
    }
    {
      char* eb = smem + w * EPI_WAVE;
      const int c4 = (lane & 7) * 4;
#pragma unroll
      for (int tn = 0; tn < 2; ++tn) {
        const int n = bn + wn * 64 + tn * 32 + c4;
        const float4 rs = ep_rs[tn], bv = ep_bv[tn];
#pragma unroll
        for (int tm = 0; tm < 4; ++tm) {
#pragma unroll
          for (int e = 0; e < 4; ++e) {
            *reinterpret_cast<float*>(eb + (4 * q4 + e) * 144 + l15 * 4) = acc[tm][2 * tn][e];
            *reinterpret_cast<float*>(eb + (4 * q4 + e) * 144 + (16 + l15) * 4) = acc[tm][2 * tn + 1][e];
          }
#pragma unroll
          for (int it = 0; it < 2; ++it) {
            const int r16 = it * 8 + (lane >> 3);
            const float4 v = *reinterpret_cast<const float4*>(eb + r16 * 144 + c4 * 4);
            const int m = bm + wm * 64 + tm * 16 + r16;
            float4 o;
            o.x = v.x * rs.x + bv.x; o.y = v.y * rs.y + bv.y; o.z = v.z * rs.z + bv.z; o.w = v.w * rs.w + bv.w;
            if (EPI == 1) { o.x = gelu_erf(o.x); o.y = gelu_erf(o.y); o.z = gelu_erf(o.z); o.w = gelu_erf(o.w); }
            float* dst = g.y + (int64_t)m * g.N + n;
            if (n < g.N && m < g.M) {
              if constexpr (!RAG) *reinterpret_cast<float4*>(dst) = o;
              else {
                dst[0] = o.x;
                if (n + 1 < g.N) dst[1] = o.y;
                if (n + 2 < g.N) dst[2] = o.z;
                if (n + 3 < g.N) dst[3] = o.w;
              }
            }
          }
        }
      }
    }
    if (!more) break;
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier(); asm volatile("" ::: "memory");     // the slices are done with
    set_tile(nbm, nbn);
    if (nlb > 0) issue_lora(0, 0, nbm, nbn); else issue_x();
    p = pn; bm = nbm; bn = nbn;
  }
}
#undef F6_MM
#undef F6_MFMA
#undef F6_ROW0
#undef F6_ROW1
#undef F6_CLOB0
#undef F6_CLOB1

