// The bf16 epilogue of one work item of the swapped-operand LDS-DMA GEMM kernels, stated once.
// NOT a header: a statement sequence, included inside the item loop of gemm_dma_body (bf16 branch)
// and of gemm_lean_kernel (gemm.hip).  A function template with the same body compiles to other
// register, spill, LDS and occupancy figures for most instances (profiles/PERF_NOTES.md, "One
// epilogue per GEMM family"); included text compiles to exactly the code of the two hand copies
// it replaces.  It keeps the .h suffix because csrc/build.py hashes every kernels/*.h into the
// library's stamp: under another suffix an edit here would not rebuild the library.
//
// Names it takes from the enclosing scope:
//   constants   TM, TN, NW, RES, PLAIN, NOALPHA, HAS_R
//   this item   w (WorkItem), m0, n0 (the wave's first row / column), it, slot, G
//   the lane    lane, wave, g = lane >> 4
//   the call    p (GemmArgs), relu, has_bias, bias_f32, st_sc1, psum_on, rc (descriptor of C)
//   state       acc[TM][TN] (C^T blocks: the lane holds C[16 ii + (lane & 15)][16 j + 4 g + 0..3]),
//               tsum (0 on entry)
// What it reads: acc, p.alpha (RES 0 - 2), the bias (has_bias: f32 or bf16, as 16-byte loads
// where the bias rows are aligned), the operand R (RES 1 / 2) through a descriptor of its own.
// Per value, in this order: alpha, bias, ReLU, apply_res8, the bf16 pack; psum_on adds the
// STORED bf16 values into tsum.  RES 3 (PLAIN) is pair exchange, pack, store; RES 4 has alpha 1.
// What it leaves: every accumulator zero and tsum 0.  Per lane exactly S_EPI = TM * TN / 2 buffer
// stores (a lane whose row or column is past M / N stores to an out-of-range offset, which the
// range check drops), and one more global store from lane 0 when psum_on: the caller's next
// counted vmcnt wait (wait_landed after an epilogue / item_start(true)) is written for exactly
// these counts.  It waits for nothing itself and touches no LDS.

// lanes g, g^1 trade halves so even g owns cols 16 j0 + 4 g .. +7 and odd g owns
// 16 j1 + 4 (g - 1) .. +7
const bool even = (g & 1) == 0;
// epilogue operand: one row block (ii) of R chunks in flight at a time (all of an item's
// chunks at once cost the second resident block its registers); rows / columns past
// M / N read 0 through the buffer range check, and the compiler's counted vmcnt waits
// for them at first use
// (two row blocks in registers: block ii + 1's loads are issued before block ii is
// processed, so only the first block's latency is exposed per item)
u32x4 rv[2][TN / 2][RES == 2 ? 2 : 1];
__amdgpu_buffer_rsrc_t rr;
if constexpr (HAS_R)
  rr = make_rsrc(p.res, (RES == 2 ? 4 : 2) * ((long)(p.batch - 1) * p.sR + (long)(p.M - 1) * p.ldr + p.N));
auto load_r = [&](int ii) {
  if constexpr (HAS_R) {
#pragma unroll
    for (int q = 0; q < TN / 2; ++q) {
      const int col = n0 + 16 * (even ? 2 * q : 2 * q + 1) + 4 * (g & ~1);
      const int row = m0 + ii * 16 + (lane & 15);
      const bool ok = row < p.M && col < p.N;
      const int off = ok ? (int)(((long)w.b * p.sR + (long)row * p.ldr + col) * (RES == 2 ? 4 : 2)) : 0x7ffffff0;
      rv[ii & 1][q][0] = __builtin_amdgcn_raw_buffer_load_b128(rr, off, 0, 0);
      if constexpr (RES == 2)
        rv[ii & 1][q][RES == 2 ? 1 : 0] = __builtin_amdgcn_raw_buffer_load_b128(rr, ok ? off + 16 : off, 0, 0);
    }
  }
};
load_r(0);
float bvs[TN / 2][8];
// bias: this lane's 8 consecutive columns as one or two 16-byte loads (aligned bias rows;
// N % 8 == 0 here) instead of 8 scalar loads of each width
const bool bias_vec = has_bias && ((((uintptr_t)p.bias) & 15) == 0) && (p.sBias % 8) == 0;
#pragma unroll
for (int q = 0; q < TN / 2; ++q) {
  const int col = n0 + 16 * (even ? 2 * q : 2 * q + 1) + 4 * (g & ~1);
  const long bo = (long)w.b * p.sBias + col;
  if (bias_vec && col + 8 <= p.N) {
    if (bias_f32) {
      const f32x4 lo = *reinterpret_cast<const f32x4*>(reinterpret_cast<const float*>(p.bias) + bo);
      const f32x4 hi = *reinterpret_cast<const f32x4*>(reinterpret_cast<const float*>(p.bias) + bo + 4);
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        bvs[q][e] = lo[e];
        bvs[q][4 + e] = hi[e];
      }
    } else {
      const u32x4 u = *reinterpret_cast<const u32x4*>(reinterpret_cast<const bf16_t*>(p.bias) + bo);
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        bvs[q][2 * e] = __uint_as_float(u[e] << 16);
        bvs[q][2 * e + 1] = __uint_as_float(u[e] & 0xffff0000u);
      }
    }
    continue;
  }
#pragma unroll
  for (int e = 0; e < 8; ++e) {
    bvs[q][e] = 0.f;
    if (has_bias && col + e < p.N) {
      bvs[q][e] = bias_f32 ? reinterpret_cast<const float*>(p.bias)[bo + e]
                           : bf2f(reinterpret_cast<const bf16_t*>(p.bias)[bo + e]);
    }
  }
}
#pragma unroll
for (int ii = 0; ii < TM; ++ii) {
  if (ii + 1 < TM) load_r(ii + 1);
#pragma unroll
  for (int q = 0; q < TN / 2; ++q) {  // both halves of a row's 128 B back to back
    const int col = n0 + 16 * (even ? 2 * q : 2 * q + 1) + 4 * (g & ~1);
    const float* bv = bvs[q];
    const f32x4 a0 = NOALPHA ? acc[ii][2 * q] : acc[ii][2 * q] * p.alpha;
    const f32x4 a1 = NOALPHA ? acc[ii][2 * q + 1] : acc[ii][2 * q + 1] * p.alpha;
    acc[ii][2 * q] = f32x4{0.f, 0.f, 0.f, 0.f};
    acc[ii][2 * q + 1] = f32x4{0.f, 0.f, 0.f, 0.f};
    float v[8];
    pair_rows16(a0, a1, even, v);
    u32x4 pk;
    if constexpr (!PLAIN) {
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        v[e] += bv[e];
        if (relu) v[e] = fmaxf(v[e], 0.f);
      }
    }
    if constexpr (HAS_R) apply_res8(v, p.flags, rv[ii & 1][q][0], rv[ii & 1][q][0], rv[ii & 1][q][RES == 2 ? 1 : 0]);
#pragma unroll
    for (int e = 0; e < 4; ++e) pk[e] = pack_bf16x2(v[2 * e], v[2 * e + 1]);
    const int row = m0 + ii * 16 + (lane & 15);
    const bool ok = row < p.M && col < p.N;  // N % 8 == 0 (launcher): chunks are whole
    const int off = ok ? (int)(((long)w.b * p.sC + (long)row * p.ldc + col) * 2) : 0x7ffffff0;
    if (st_sc1) __builtin_amdgcn_raw_buffer_store_b128(pk, rc, off, 0, kSC1);
    else __builtin_amdgcn_raw_buffer_store_b128(pk, rc, off, 0, 0);
    if (psum_on && ok) {
#pragma unroll
      for (int e = 0; e < 4; ++e) tsum += __uint_as_float(pk[e] << 16) + __uint_as_float(pk[e] & 0xffff0000u);
    }
  }
}
if (psum_on) {
  // fused loss reduction: this wave's share of sum(C) -- of the bf16 values just stored --
  // to its own slot (one store per wave, counted in the next K-step's vmcnt)
  tsum = warp_sum64(tsum);
  if (lane == 0) p.psum[(long)(slot + G * it) * NW + wave] = tsum;
  tsum = 0.f;
}
