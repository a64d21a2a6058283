// Batched bf16 GEMM on CDNA4 MFMA (v_mfma_f32_16x16x32_bf16), f32 accumulation.
//
//   C[b] = alpha * op(A[b]) @ op(B[b]) (+ bias) (relu)        (bf16 or f32 out, optional split-K)
//
// Operand layouts (template flags), covering every GEMM of the attention block's
// forward and backward without transposing anything in memory:
//   A_KC : A[m][k] at A + m*lda + k   (k contiguous)      | !A_KC : A[m][k] at A + k*lda + m
//   B_KC : B[k][n] at B + n*ldb + k   (k contiguous)      | !B_KC : B[k][n] at B + k*ldb + n
// k-contiguous operands are staged as [rows][64] LDS tiles read with ds_read_b128;
// m/n-contiguous operands as [64][rows] tiles read with the gfx950 transposing LDS read
// (ds_read_b64_tr_b16), so e.g. dW = X^T @ dY reads X and dY in their natural layouts.
//
// Structure: 256 threads = 4 waves (2x2), block tile BM x BN, BK = 64, LDS double buffer
// with register staging (issue next tile's global loads before the MFMAs, write them to
// the other LDS buffer after; one barrier per K-tile), XOR-swizzled LDS images so both
// the row reads and the transposed reads are bank-conflict free, XCD-aware tile order.
#include "common.h"
#include <stdio.h>
#include <stdlib.h>
#include <type_traits>

namespace {

constexpr int BK = 64;

struct GemmArgs {
  const bf16_t* A;
  const bf16_t* B;
  void* C;
  const void* bias;
  long lda, ldb, ldc;
  long sA, sB, sC, sBias;
  int M, N, K;
  int batch, splitk, kt_per_split;
  float alpha;
  int flags;  // 1 relu, 2 bias, 4 bias f32, 8 accumulate into C (f32 out); epilogue operand R
              // (bf16 output only): 64 residual add, 128 ReLU mask (keep where R > 0), 256 R is f32
  float* psum;  // LDS-DMA kernels, bf16 out: per (item, wave) sums of the stored values, or null
  const void* res;  // R[b][row][col] at res + b * sR + row * ldr + col (ldr may be 0: one broadcast row)
  long ldr, sR;
  const bf16_t* bptr[4];  // flags & kBPtrs (slab mode): batch b's B operand (instead of B + b * sB)
  unsigned long long* trace;  // LJS_GEMM_TRACE builds only: per-wave timestamps (see gemm_trace)
};

// Transposed fragment reads as asm statements, for a K-loop that keeps LDS-DMA pieces in flight
// across its barrier.  The compiler knows nothing about what ds_read_tr16_b64 (the builtin) reads,
// so with a DMA outstanding it puts s_waitcnt vmcnt(0) in front of every group of them: every
// m/n-contiguous LDS-DMA kernel drains its ring right after the barrier, whatever its counted wait
// said (the k-contiguous kernels' plain ds_read_b128 are not treated so).  An asm read is not
// counted by the compiler at all, so these come with their own lgkmcnt waits:
//   tr_read5_wait   5 fragments, valid when the statement ends (it waits lgkmcnt(0) itself);
//   tr_read3 / 4    fragments that are NOT valid until a tr_wait* statement naming them ("+v", so
//                   nothing that uses them can be scheduled above it) -- join the halves into an
//                   MFMA operand only after that, so that a register copy the join may need reads
//                   landed data.
// A fragment is two reads 4 k-rows (1024 B at 128-wide rows) apart from one address; ad: LDS byte
// addresses (frag_tr_addr below).
#define LJS_TR2(l, h, a) "ds_read_b64_tr_b16 %" #l ", %" #a "\n\tds_read_b64_tr_b16 %" #h ", %" #a " offset:1024\n\t"
__device__ __forceinline__ void tr_read5_wait(s16x4* lo, s16x4* hi, const unsigned* ad) {
  asm volatile(LJS_TR2(0, 1, 10) LJS_TR2(2, 3, 11) LJS_TR2(4, 5, 12) LJS_TR2(6, 7, 13) LJS_TR2(8, 9, 14)
               "s_waitcnt lgkmcnt(0)"
               : "=&v"(lo[0]), "=&v"(hi[0]), "=&v"(lo[1]), "=&v"(hi[1]), "=&v"(lo[2]), "=&v"(hi[2]), "=&v"(lo[3]),
                 "=&v"(hi[3]), "=&v"(lo[4]), "=&v"(hi[4])
               : "v"(ad[0]), "v"(ad[1]), "v"(ad[2]), "v"(ad[3]), "v"(ad[4])
               : "memory");
}
__device__ __forceinline__ void tr_read3(s16x4* lo, s16x4* hi, const unsigned* ad) {
  asm volatile(LJS_TR2(0, 1, 6) LJS_TR2(2, 3, 7) LJS_TR2(4, 5, 8)
               : "=&v"(lo[0]), "=&v"(hi[0]), "=&v"(lo[1]), "=&v"(hi[1]), "=&v"(lo[2]), "=&v"(hi[2])
               : "v"(ad[0]), "v"(ad[1]), "v"(ad[2])
               : "memory");
}
__device__ __forceinline__ void tr_read4(s16x4* lo, s16x4* hi, const unsigned* ad) {
  asm volatile(LJS_TR2(0, 1, 8) LJS_TR2(2, 3, 9) LJS_TR2(4, 5, 10) LJS_TR2(6, 7, 11)
               : "=&v"(lo[0]), "=&v"(hi[0]), "=&v"(lo[1]), "=&v"(hi[1]), "=&v"(lo[2]), "=&v"(hi[2]), "=&v"(lo[3]),
                 "=&v"(hi[3])
               : "v"(ad[0]), "v"(ad[1]), "v"(ad[2]), "v"(ad[3])
               : "memory");
}
#undef LJS_TR2
#define LJS_TRW(x, i) "+v"(x##lo[i]), "+v"(x##hi[i])
// every read issued so far has landed: the 3 fragments of a (tr_read3) and the 8 of b (2 x tr_read4)
__device__ __forceinline__ void tr_wait3_8(s16x4* alo, s16x4* ahi, s16x4* blo, s16x4* bhi) {
  asm volatile("s_waitcnt lgkmcnt(0)"
               : LJS_TRW(a, 0), LJS_TRW(a, 1), LJS_TRW(a, 2), LJS_TRW(b, 0), LJS_TRW(b, 1), LJS_TRW(b, 2),
                 LJS_TRW(b, 3), LJS_TRW(b, 4), LJS_TRW(b, 5), LJS_TRW(b, 6), LJS_TRW(b, 7)
               :
               : "memory");
}
#undef LJS_TRW

// Timeline instrumentation of the LDS-DMA kernel (compiled in with -DLJS_GEMM_TRACE only, a
// variant library for scripts/gemm_trace.py): per wave, kTraceSlots core-clock stamps (s_memtime)
// written by lane 0 with vector stores -- kernel start, then per K-tile wait: before the counted
// vmcnt, after it, after the barrier -- and the end.
constexpr int kTraceSlots = 128;

constexpr int kResAdd = 64, kResMask = 128, kResF32 = 256;
// f32 output, m/n-contiguous operands, batch 1: split s writes its own slab C + s * sC (no
// atomics; summed by slab_reduce) and the splits need not divide the K-tiles -- the last one
// runs past K, where the buffer range check reads zeros
constexpr int kSlabs = 512;
// item order with the tile-row fastest (set by the launcher when there are fewer tile rows
// than tile columns; see decode_item)
constexpr int kMFast = 1024;
// B operand of batch b taken from bptr[b] (up to 4 separate tensors, e.g. the q / k / v
// cotangents of a weight-major fused projection) -- slab-mode LDS-DMA kernels only
constexpr int kBPtrs = 4096;
// slab mode, the block's LAST item: its f32 tile leaves through the (then idle) LDS ring as whole
// 256-byte rows (16-byte chunk XOR row), not as 64-byte pieces of 16 rows per store instruction
constexpr int kSlabVst = 8192;

// Epilogue operand R applied to 8 consecutive output values (after bias / ReLU, f32):
//   residual add: out = bf16(bf16(v) + bf16(R))   (the unfused "y = dense(x); y + R" in bf16:
//                 both roundings kept, so the fusion is bit-exact)
//   ReLU mask   : out = R > 0 ? v : 0             (the ReLU backward of a dense whose input R is a
//                 ReLU output, fused into the dX GEMM producing v)
// rb holds R's 8 values as bf16 pairs (bf16 R) or rf their f32 values (f32 R).
__device__ __forceinline__ void apply_res8(float* v, int flags, const u32x4& rb, const u32x4& rf0,
                                           const u32x4& rf1) {
  float r[8];
  if (flags & kResF32) {
#pragma unroll
    for (int e = 0; e < 4; ++e) { r[e] = __uint_as_float(rf0[e]); r[4 + e] = __uint_as_float(rf1[e]); }
  } else {
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      r[2 * e] = __uint_as_float(rb[e] << 16);
      r[2 * e + 1] = __uint_as_float(rb[e] & 0xffff0000u);
    }
  }
  if (flags & kResAdd) {
#pragma unroll
    for (int e = 0; e < 8; ++e) v[e] = bf2f(f2bf(v[e])) + bf2f(f2bf(r[e]));
  } else if (flags & kResMask) {
#pragma unroll
    for (int e = 0; e < 8; ++e) v[e] = r[e] > 0.f ? v[e] : 0.f;
  }
}

// swizzled 8-byte-chunk index for the m/n-contiguous image (rows of R bf16)
template <int R>
__device__ __forceinline__ int swz_mn(int krow, int c8) {
  int f;
  if constexpr (R >= 128) f = ((krow & 3) | (((krow >> 3) & 1) << 2)) << 2;
  else f = ((((krow >> 1) & 1)) | (((krow >> 3) & 1) << 1)) << 2;
  return c8 ^ f;
}

// swizzled 16-byte-chunk index for the k-contiguous image (rows of 64 bf16 = 8 chunks)
__device__ __forceinline__ int swz_k(int row, int c16) { return c16 ^ ((row >> 1) & 7); }

template <int R, bool KC>
struct Stage {
  static constexpr int CHUNKS = R * BK * 2 / 16 / 256;  // 16-byte chunks per thread
  u32x4 v[CHUNKS];

  __device__ __forceinline__ void load(const bf16_t* __restrict__ base, long ld, int r0, int k0, int R_lim,
                                       int K, int tid) {
#pragma unroll
    for (int i = 0; i < CHUNKS; ++i) {
      int c = tid + 256 * i;
      if constexpr (KC) {
        int row = c >> 3, kc = c & 7;
        int gr = r0 + row, gk = k0 + kc * 8;
        if (gr < R_lim && gk < K)
          v[i] = *reinterpret_cast<const u32x4*>(base + (long)gr * ld + gk);
        else
          v[i] = u32x4{0, 0, 0, 0};
      } else {
        constexpr int CPR = R / 8;  // 16B chunks per k-row
        int krow = c / CPR, mc = c % CPR;
        int gk = k0 + krow, gr = r0 + mc * 8;
        if (gk < K && gr < R_lim)
          v[i] = *reinterpret_cast<const u32x4*>(base + (long)gk * ld + gr);
        else
          v[i] = u32x4{0, 0, 0, 0};
      }
    }
  }

  __device__ __forceinline__ void store(bf16_t* lds, int tid) const {
#pragma unroll
    for (int i = 0; i < CHUNKS; ++i) {
      int c = tid + 256 * i;
      if constexpr (KC) {
        int row = c >> 3, kc = c & 7;
        *reinterpret_cast<u32x4*>(lds + row * BK + swz_k(row, kc) * 8) = v[i];
      } else {
        constexpr int CPR = R / 8;
        int krow = c / CPR, mc = c % CPR;
        *reinterpret_cast<u32x4*>(lds + krow * R + swz_mn<R>(krow, mc * 2) * 4) = v[i];
      }
    }
  }
};

// MFMA operand fragment: 16 rows (m or n) starting at rb, k-step ks (32 deep)
template <int R, bool KC>
__device__ __forceinline__ bf16x8 frag(const bf16_t* lds, int rb, int ks, int lane) {
  if constexpr (KC) {
    int row = rb + (lane & 15);
    int kc = ks * 4 + (lane >> 4);
    u32x4 raw = *reinterpret_cast<const u32x4*>(lds + row * BK + swz_k(row, kc) * 8);
    return __builtin_bit_cast(bf16x8, raw);
  } else {
    int g = lane >> 4, i = lane & 15, q = i >> 2, p = i & 3;
    int kr0 = ks * 32 + 8 * g + q;
    int c8 = (rb >> 2) + p;
    s16x4 lo = lds_read_tr16(lds + kr0 * R + swz_mn<R>(kr0, c8) * 4);
    int kr1 = kr0 + 4;
    s16x4 hi = lds_read_tr16(lds + kr1 * R + swz_mn<R>(kr1, c8) * 4);
    return join_bf16x8(lo, hi);
  }
}

// LDS byte address of the first read of frag<128, false>(lds, rb, 0, lane), for the tr_read* statements
__device__ __forceinline__ unsigned frag_tr_addr(const bf16_t* lds, int rb, int lane) {
  const int g = lane >> 4, i = lane & 15, q = i >> 2, p = i & 3;
  const int kr0 = 8 * g + q;
  const int c8 = (rb >> 2) + p;
  return (unsigned)(unsigned long)(LDS_PTR(const bf16_t))(lds + kr0 * 128 + swz_mn<128>(kr0, c8) * 4);
}

template <int BM, int BN, bool A_KC, bool B_KC, bool OUT_F32>
__global__ __launch_bounds__(256) void gemm_bf16_kernel(GemmArgs p) {
  constexpr int TM = BM / 32, TN = BN / 32;  // 16x16 MFMA tiles per wave (2x2 waves)
  constexpr int A_TILE = BM * BK, B_TILE = BN * BK;
  __shared__ __attribute__((aligned(16))) bf16_t smem[2 * (A_TILE + B_TILE)];
  // (pointer arrays into LDS would become static initializers: index arithmetically)
#define As(i) (smem + (i) * A_TILE)
#define Bs(i) (smem + 2 * A_TILE + (i) * B_TILE)

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wr = wave >> 1, wc = wave & 1;
  const int ntm = (p.M + BM - 1) / BM, ntn = (p.N + BN - 1) / BN;
  const int tile = xcd_remap(blockIdx.x, gridDim.x);
  const int tm_i = tile / ntn, tn_i = tile % ntn;
  if (tm_i >= ntm) return;
  const int bz = blockIdx.y;
  const int b = bz / p.splitk, split = bz % p.splitk;
  const int m0 = tm_i * BM, n0 = tn_i * BN;

  const bf16_t* Ab = p.A + (long)b * p.sA;
  const bf16_t* Bb = p.B + (long)b * p.sB;

  const int nkt_total = (p.K + BK - 1) / BK;
  const int kt_begin = split * p.kt_per_split;
  const int kt_end = min(nkt_total, kt_begin + p.kt_per_split);

  f32x4 acc[TM][TN];
#pragma unroll
  for (int i = 0; i < TM; ++i)
#pragma unroll
    for (int j = 0; j < TN; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};

  Stage<BM, A_KC> sa;
  Stage<BN, B_KC> sb;
  if (kt_begin < kt_end) {
    sa.load(Ab, p.lda, m0, kt_begin * BK, p.M, p.K, tid);
    sb.load(Bb, p.ldb, n0, kt_begin * BK, p.N, p.K, tid);
    sa.store(As(0), tid);
    sb.store(Bs(0), tid);
  }
  __syncthreads();

  for (int kt = kt_begin; kt < kt_end; ++kt) {
    const int cur = (kt - kt_begin) & 1;
    const bool more = kt + 1 < kt_end;
    if (more) {
      sa.load(Ab, p.lda, m0, (kt + 1) * BK, p.M, p.K, tid);
      sb.load(Bb, p.ldb, n0, (kt + 1) * BK, p.N, p.K, tid);
    }
#pragma unroll
    for (int ks = 0; ks < BK / 32; ++ks) {
      bf16x8 af[TM], bfr[TN];
#pragma unroll
      for (int i = 0; i < TM; ++i) af[i] = frag<BM, A_KC>(As(cur), wr * (BM / 2) + i * 16, ks, lane);
#pragma unroll
      for (int j = 0; j < TN; ++j) bfr[j] = frag<BN, B_KC>(Bs(cur), wc * (BN / 2) + j * 16, ks, lane);
#pragma unroll
      for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int j = 0; j < TN; ++j) acc[i][j] = mfma16x16x32(af[i], bfr[j], acc[i][j]);
    }
    if (more) {
      sa.store(As(cur ^ 1), tid);
      sb.store(Bs(cur ^ 1), tid);
    }
    __syncthreads();
  }

  // ---------------------------------------------------------------- epilogue
  const bool relu = p.flags & 1;
  const bool has_bias = (p.flags & 2) && p.splitk == 1;
  const bool bias_f32 = p.flags & 4;
  const bool accumulate = p.flags & 8;
  if constexpr (!OUT_F32) {
    // bf16 output: stage the tile in LDS (the K loop's last barrier freed it), then write whole
    // rows with 16-byte stores instead of 2-byte scattered accumulator-layout stores.
    constexpr int LDC = BN + 8;
    bf16_t* ct = smem;
#pragma unroll
    for (int j = 0; j < TN; ++j) {
      const int cl = wc * (BN / 2) + j * 16 + (lane & 15);
      const int col = n0 + cl;
      float bv = 0.f;
      if (has_bias && col < p.N) {
        const long bo = (long)b * p.sBias + col;
        bv = bias_f32 ? reinterpret_cast<const float*>(p.bias)[bo]
                      : bf2f(reinterpret_cast<const bf16_t*>(p.bias)[bo]);
      }
#pragma unroll
      for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          float v = acc[i][j][r] * p.alpha + bv;
          if (relu) v = fmaxf(v, 0.f);
          ct[(wr * (BM / 2) + i * 16 + (lane >> 4) * 4 + r) * LDC + cl] = f2bf(v);
        }
    }
    __syncthreads();
    bf16_t* Cb = reinterpret_cast<bf16_t*>(p.C) + (long)b * p.sC;
    constexpr int CPR = BN / 8;
    const bool vec_ok = (p.ldc % 8 == 0) && ((((uintptr_t)Cb) & 15) == 0);
    for (int c = tid; c < BM * CPR; c += 256) {
      const int rl = c / CPR, cc = c % CPR;
      const int row = m0 + rl, col = n0 + cc * 8;
      if (row >= p.M || col >= p.N) continue;
      const bf16_t* src = ct + rl * LDC + cc * 8;
      bf16_t* dst = Cb + (long)row * p.ldc + col;
      if (p.flags & (kResAdd | kResMask)) {
        float v[8];
        u32x4 rb = {0, 0, 0, 0}, rf0 = {0, 0, 0, 0}, rf1 = {0, 0, 0, 0};
        const long ro = (long)b * p.sR + (long)row * p.ldr + col;
#pragma unroll
        for (int e = 0; e < 8; ++e) {
          v[e] = bf2f(src[e]);
          if (col + e < p.N) {
            if (p.flags & kResF32) {
              const float rv = reinterpret_cast<const float*>(p.res)[ro + e];
              if (e < 4) rf0[e] = __float_as_uint(rv); else rf1[e - 4] = __float_as_uint(rv);
            } else {
              const unsigned rv = reinterpret_cast<const bf16_t*>(p.res)[ro + e];
              rb[e >> 1] |= (e & 1) ? (rv << 16) : rv;
            }
          }
        }
        apply_res8(v, p.flags, rb, rf0, rf1);
        if (vec_ok && col + 8 <= p.N)
          *reinterpret_cast<u32x4*>(dst) = u32x4{pack_bf16x2(v[0], v[1]), pack_bf16x2(v[2], v[3]),
                                                 pack_bf16x2(v[4], v[5]), pack_bf16x2(v[6], v[7])};
        else
          for (int e = 0; e < 8 && col + e < p.N; ++e) dst[e] = f2bf(v[e]);
      } else if (vec_ok && col + 8 <= p.N) {
        *reinterpret_cast<u32x4*>(dst) = *reinterpret_cast<const u32x4*>(src);
      } else {
        for (int e = 0; e < 8 && col + e < p.N; ++e) dst[e] = src[e];
      }
    }
    return;
  }
#pragma unroll
  for (int i = 0; i < TM; ++i) {
#pragma unroll
    for (int j = 0; j < TN; ++j) {
      const int col = n0 + wc * (BN / 2) + j * 16 + (lane & 15);
      if (col >= p.N) continue;
      float bv = 0.f;
      if (has_bias) {
        const long bo = (long)b * p.sBias + col;
        bv = bias_f32 ? reinterpret_cast<const float*>(p.bias)[bo]
                      : bf2f(reinterpret_cast<const bf16_t*>(p.bias)[bo]);
      }
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int row = m0 + wr * (BM / 2) + i * 16 + (lane >> 4) * 4 + r;
        if (row >= p.M) continue;
        float v = acc[i][j][r] * p.alpha + bv;
        if (relu) v = fmaxf(v, 0.f);
        const long off = (long)b * p.sC + (long)row * p.ldc + col;
        if constexpr (OUT_F32) {
          float* C = reinterpret_cast<float*>(p.C);
          if (p.splitk > 1) atomicAdd(C + off, v);
          else if (accumulate) C[off] += v;
          else C[off] = v;
        } else {
          reinterpret_cast<bf16_t*>(p.C)[off] = f2bf(v);
        }
      }
    }
  }
}

#undef As
#undef Bs

// ============================================================================ LDS-DMA GEMM
// Persistent, pipelined MFMA GEMM for the large bench shapes.
//  * Staging by the buffer LDS-DMA (buffer_load_dwordx4 ... lds): global -> LDS with no VGPRs
//    and no ds_write (the VGPR->LDS transfer, ~79 B/clk/CU, bounds a register-staged loop).
//    Swizzles are applied on the SOURCE address (the DMA writes a wave's 64 x 16 B
//    contiguously), so the LDS images are those of the kernel above (conflict-free reads).
//  * Persistent blocks walk a FLATTENED (work item, K-tile) sequence through an NST-deep LDS
//    ring with one raw s_barrier per K-tile and a counted vmcnt, so the next item's first
//    tiles are already in flight while the current item's epilogue runs: no per-tile
//    prologue bubble (K = 512/640 projections have only 8-10 K-tiles per item).
//  * The MFMA operands are swapped (C^T = B^T A^T per 16x16 block), so each lane ends with 4
//    CONSECUTIVE columns of one output row: bf16 results leave as packed 8-byte stores and
//    f32 as 16-byte stores straight from the accumulators (no LDS round trip).
//  * Work items are ordered (split, batch, tiles; the dimension of fewer tiles fastest) and
//    dealt XCD-aware, so blocks sharing an XCD's L2 work on neighbouring tiles (shared panels).
// Edges: rows/cols past M/N read garbage that only reaches discarded outputs; the buffer
// descriptor's range check turns every out-of-range read into 0 without faulting; K must be a
// multiple of 64 and the split must divide the K-tiles (checked by the launcher) except in
// slab mode (kSlabs), whose last split reads zeros past K.

// XOR applied to the 16-byte chunk index of k-row `krow` of an m/n-contiguous image (R rows)
template <int R>
__device__ __forceinline__ int swz_mn16(int krow) {
  // (rows of 128 or 256 bf16 start on the same bank; rows of 64 alternate halves)
  if constexpr (R >= 128) return ((krow & 3) | (((krow >> 3) & 1) << 2)) << 1;
  else return ((((krow >> 1) & 1)) | (((krow >> 3) & 1) << 1)) << 1;
}


// s_waitcnt vmcnt with a wave-uniform runtime count (a jump over immediates; counts above 47
// wait for 47, which is only stricter)
template <int N>
__device__ __forceinline__ void wait_vm_imm() {
  asm volatile("s_waitcnt vmcnt(%0)" ::"n"(N) : "memory");
}
__device__ __forceinline__ void wait_vm_n(int n) {
  switch (n) {
#define LJS_W(k) case k: wait_vm_imm<k>(); return;
    LJS_W(0) LJS_W(1) LJS_W(2) LJS_W(3) LJS_W(4) LJS_W(5) LJS_W(6) LJS_W(7) LJS_W(8) LJS_W(9) LJS_W(10)
    LJS_W(11) LJS_W(12) LJS_W(13) LJS_W(14) LJS_W(15) LJS_W(16) LJS_W(17) LJS_W(18) LJS_W(19) LJS_W(20)
    LJS_W(21) LJS_W(22) LJS_W(23) LJS_W(24) LJS_W(25) LJS_W(26) LJS_W(27) LJS_W(28) LJS_W(29) LJS_W(30)
    LJS_W(31) LJS_W(32) LJS_W(33) LJS_W(34) LJS_W(35) LJS_W(36) LJS_W(37) LJS_W(38) LJS_W(39) LJS_W(40)
    LJS_W(41) LJS_W(42) LJS_W(43) LJS_W(44) LJS_W(45) LJS_W(46)
#undef LJS_W
    default: wait_vm_imm<47>(); return;
  }
}

// One operand tile (R rows x BK) of one K-tile: its 1 KiB DMA pieces, split over NW waves.
// Per-lane offsets are relative to (row 0, k 0); the tile origin goes in the scalar offset.
template <int R, bool KC, int NW>
struct DmaTile {
  static constexpr int PIECES = R * BK * 2 / 1024;
  static constexpr int PER_WAVE = PIECES / NW;
  static_assert(PIECES % NW == 0, "pieces must split evenly over the waves");
  int voff[PER_WAVE];

  __device__ __forceinline__ void init(long ld, int wave, int lane) {
#pragma unroll
    for (int i = 0; i < PER_WAVE; ++i) {
      const int q = wave + NW * i;
      long e;
      if constexpr (KC) {
        const int row = 8 * q + (lane >> 3), slot = lane & 7;
        e = (long)row * ld + 8 * (slot ^ ((row >> 1) & 7));
      } else {
        constexpr int CPR = R / 8;     // 16 B chunks per k-row
        constexpr int KPP = 64 / CPR;  // k-rows per piece
        const int krow = KPP * q + lane / CPR, slot = lane % CPR;
        e = (long)krow * ld + 8 * (slot ^ swz_mn16<R>(krow));
      }
      voff[i] = (int)(e * 2);
    }
  }

  // soff: byte offset of the tile origin (row r0, k-tile kt), wave-uniform
  __device__ __forceinline__ void issue(__amdgpu_buffer_rsrc_t rs, bf16_t* lds, int soff, int wave) const {
#pragma unroll
    for (int i = 0; i < PER_WAVE; ++i)
      __builtin_amdgcn_raw_ptr_buffer_load_lds(rs, (LDS_PTR(void))(lds + (wave + NW * i) * 512), 16, voff[i], soff,
                                               0, 0);
  }

  // half H of the tile (its k-rows 32 H .. 32 H + 31 -- an m/n-contiguous wave's pieces 2 H and
  // 2 H + 1 when every piece is 4 k-rows and 4 waves share the tile) into a half-tile image at lds
  template <int H>
  __device__ __forceinline__ void issue_half(__amdgpu_buffer_rsrc_t rs, bf16_t* lds, int soff, int wave) const {
    static_assert(!KC && PER_WAVE == 4 && R == 128, "pieces i and i + 2 are 32 k-rows apart");
#pragma unroll
    for (int i = 0; i < 2; ++i)
      __builtin_amdgcn_raw_ptr_buffer_load_lds(rs, (LDS_PTR(void))(lds + (wave + NW * i) * 512), 16, voff[2 * H + i],
                                               soff, 0, 0);
  }
};

struct WorkItem {
  int b, m0, n0, kt0, split;
};

// item order (split, batch, tile-row, tile-col) with the dimension of FEWER tiles fastest: with
// the XCD-aware deal an XCD's blocks then share one K-range (split) and cover a compact block
// of tiles -- all of the narrow operand's panels and a slice of the wide one's -- so its L2
// holds both (the FF weight gradient dW_in [640 x 2560] read every dA panel on every XCD with
// the tile-col-fastest order: 80 us vs 63 for the transposed dW_out)
__device__ __forceinline__ WorkItem decode_item(const GemmArgs& p, int item, int ntm, int ntn) {
  WorkItem w;
  int tm_i, tn_i, r;
  if (p.flags & kMFast) {
    tm_i = item % ntm;
    r = item / ntm;
    tn_i = r % ntn;
    r /= ntn;
  } else {
    tn_i = item % ntn;
    r = item / ntn;
    tm_i = r % ntm;
    r /= ntm;
  }
  w.b = r % p.batch;
  w.split = r / p.batch;
  w.m0 = tm_i;
  w.n0 = tn_i;
  w.kt0 = w.split * p.kt_per_split;
  return w;
}

constexpr int kSC1 = 16;  // buffer-instruction cache policy bit: sc1 (gfx940-family CPol::SC1)

// RES: epilogue operand R (bf16 output only; see apply_res8): 0 none, 1 bf16 R, 2 f32 R.  A
// template parameter so kernels without it keep their register allocation.
// (a 4-wave kernel whose LDS ring lets two blocks share a CU is told so: the pipelined main loop's
// second fragment set and the epilogue registers would otherwise push VGPR + AGPR past 256 and
// halve the resident blocks)
// (the body of gemm_dma_kernel; `bid` / `G` are the block's index and the grid as far as this
// GEMM is concerned -- a grouped launch, gemm_dma_group2_kernel, runs two GEMMs' items in one grid)
template <int BM, int BN, int WM, int WN, int NST, bool A_KC, bool B_KC, bool OUT_F32, int RES = 0>
__device__ __forceinline__ void gemm_dma_body(const GemmArgs& p, const int bid, const int G) {
  constexpr int NW = WM * WN;
  constexpr int TM = BM / WM / 16, TN = BN / WN / 16;
  constexpr int A_TILE = BM * BK, B_TILE = BN * BK, STAGE = A_TILE + B_TILE;
  using TA = DmaTile<BM, A_KC, NW>;
  using TB = DmaTile<BN, B_KC, NW>;
  constexpr int L = TA::PER_WAVE + TB::PER_WAVE;   // vector-memory instructions per wave per K-tile
  // Operands swapped (C^T = B^T A^T per 16x16 block): each lane ends with 4 CONSECUTIVE
  // columns of one output row.  bf16 output: lanes pair up into 16-byte row chunks and leave
  // through exactly S_EPI buffer stores per lane (masked lanes get an out-of-range offset, so
  // the count is exact and the next K-step's counted vmcnt stays valid).  f32 output (split-K
  // slabs / atomics, weight grads): one 16-byte store (or 4 atomics) per block, full drain after.
  constexpr bool SWAP = true;
  static_assert(OUT_F32 || TN % 2 == 0, "column blocks pair up for 16-byte stores");
  constexpr int S_EPI = TM * TN / 2;
  static_assert(L * (NST - 1) + S_EPI + 1 <= 63, "vmcnt immediate range");
  // RING: the 4-wave 128x128 weight-gradient slab instance (tile code 1282) keeps its LDS as FIVE
  // HALF-tile slots (32 k-rows of A, then of B: 16 KiB each, 80 KiB -- still two blocks per CU)
  // instead of two whole stages, so halves stay in flight across every barrier.  NST = 2 then only
  // says "two whole stages' worth": it stays in the template arguments (and the launch record's
  // name) and sizes nothing here.  The schedule is at ring_wait below.
  constexpr bool RING = NST == 2 && BM == 128 && BN == 128 && NW == 4 && !A_KC && !B_KC && OUT_F32 && RES == 3;
  constexpr int HALF = STAGE / 2, A_HALF = A_TILE / 2, RING_SLOTS = 5;
  constexpr int E_RING = TM * TN;   // an item's direct f32 stores per lane (one per accumulator block)
  static_assert(!RING || 4 * L / 2 + E_RING + 1 <= 63, "vmcnt immediate range");
  __shared__ __attribute__((aligned(16))) bf16_t smem[RING ? RING_SLOTS * HALF : NST * STAGE];

  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wr = wave / WN, wc = wave % WN;
  const int ntm = (p.M + BM - 1) / BM, ntn = (p.N + BN - 1) / BN;
  const int items = p.batch * p.splitk * ntm * ntn;
  const int slot = xcd_remap(bid, G);   // same-XCD blocks take neighbouring items
  const int my_items = slot < items ? (items - slot + G - 1) / G : 0;
  const int nk = p.kt_per_split;               // K-tiles per item (the split divides them)
  const int total = my_items * nk;
#ifdef LJS_GEMM_TRACE
  unsigned long long* trc = p.trace ? p.trace + ((long)bid * NW + wave) * kTraceSlots : nullptr;
  int trn = 0;
  auto stamp = [&]() {
    if (trc && trn < kTraceSlots - 1) {
      const unsigned long long t = __builtin_amdgcn_s_memtime();
      if (lane == 0) trc[trn] = t;
    }
    ++trn;
  };
  auto stamp_end = [&]() {
    if (trc) {
      const unsigned long long t = __builtin_amdgcn_s_memtime();
      if (lane == 0) trc[kTraceSlots - 1] = t;
    }
  };
  // stamp(), and whether it stored: a stamp is one more entry of the wave's vmcnt queue
  auto stamp_st = [&]() {
    const int st = trc && trn < kTraceSlots - 1;
    stamp();
    return st;
  };
#else
  auto stamp = [&]() {};
  auto stamp_end = [&]() {};
  auto stamp_st = [&]() { return 0; };
#endif
  stamp();

  constexpr int AES = 2;  // A element bytes
  const long a_bytes = AES * (A_KC ? (long)(p.M - 1) * p.lda + p.K : (long)(p.K - 1) * p.lda + p.M);
  const long b_bytes = 2 * (B_KC ? (long)(p.N - 1) * p.ldb + p.K : (long)(p.K - 1) * p.ldb + p.N);
  const long a_kt = A_KC ? (long)BK * AES : (long)BK * p.lda * 2;  // bytes per K-tile step
  const long b_kt = B_KC ? (long)BK * 2 : (long)BK * p.ldb * 2;

  TA ta;
  TB tb;
  ta.init(p.lda, wave, lane);
  tb.init(p.ldb, wave, lane);

  // issue-side cursor: the item whose K-tiles are being fetched, advanced incrementally with
  // 32-bit scalar offsets (the launcher guarantees operand extents < 2^30 bytes)
  int is_item = 0, is_kt = 0;
  __amdgpu_buffer_rsrc_t ra, rb;
  int a_off = 0, b_off = 0;
  const int a_step = (int)a_kt, b_step = (int)b_kt;
  auto load_item = [&](int k) {
    const WorkItem w = decode_item(p, slot + G * k, ntm, ntn);
    ra = make_rsrc(reinterpret_cast<const unsigned char*>(p.A) + (long)w.b * p.sA * AES, a_bytes);
    rb = make_rsrc((p.flags & kBPtrs) ? p.bptr[w.b] : p.B + (long)w.b * p.sB, b_bytes);
    a_off = __builtin_amdgcn_readfirstlane(
        (int)((A_KC ? (long)w.m0 * BM * p.lda : (long)w.m0 * BM) * AES + w.kt0 * a_kt));
    b_off = __builtin_amdgcn_readfirstlane(
        (int)((B_KC ? (long)w.n0 * BN * p.ldb : (long)w.n0 * BN) * 2 + w.kt0 * b_kt));
  };
  auto issue_a = [&](int st) { ta.issue(ra, smem + st * STAGE, a_off, wave); };
  auto issue_b = [&](int st) { tb.issue(rb, smem + st * STAGE + A_TILE, b_off, wave); };
  auto issue_next = [&](int st) {
    if (is_kt == 0) load_item(is_item);
    issue_a(st);
    issue_b(st);
    a_off += a_step;
    b_off += b_step;
    if (++is_kt == nk) { is_kt = 0; ++is_item; }
  };
  // the same in two halves (A pieces, then B pieces + cursor advance)
  auto issue_half = [&](int st, bool second) {
    if (!second) {
      if (is_kt == 0) load_item(is_item);
      issue_a(st);
      a_off += a_step;
    } else {
      issue_b(st);
      b_off += b_step;
      if (++is_kt == nk) { is_kt = 0; ++is_item; }
    }
  };

  f32x4 acc[TM][TN];
#pragma unroll
  for (int i = 0; i < TM; ++i)
#pragma unroll
    for (int j = 0; j < TN; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};

  // RING: the halves of the flattened (item, K-tile) sequence are numbered h = 0, 1, 2, ... (tile f
  // is halves 2 f and 2 f + 1) and issued strictly in that order, half h into slot h mod 5: the
  // write slot just rotates.  A half is 2 A pieces and 2 B pieces per wave (L / 2 = 4 instructions).
  int ring_w = 0, ring_r = 0;   // element offsets of the next half's slot / of tile f's first half
  auto ring_adv = [](int so, int n) {
    so += n * HALF;
    return so >= RING_SLOTS * HALF ? so - RING_SLOTS * HALF : so;
  };
  auto ring_issue0 = [&]() {   // k-rows 0-31 of the cursor's tile
    if constexpr (RING) {
      if (is_kt == 0) load_item(is_item);
      ta.template issue_half<0>(ra, smem + ring_w, a_off, wave);
      tb.template issue_half<0>(rb, smem + ring_w + A_HALF, b_off, wave);
      ring_w = ring_adv(ring_w, 1);
    }
  };
  auto ring_issue1 = [&]() {   // k-rows 32-63, and the cursor moves on
    if constexpr (RING) {
      ta.template issue_half<1>(ra, smem + ring_w, a_off, wave);
      tb.template issue_half<1>(rb, smem + ring_w + A_HALF, b_off, wave);
      ring_w = ring_adv(ring_w, 1);
      a_off += a_step;
      b_off += b_step;
      if (++is_kt == nk) { is_kt = 0; ++is_item; }
    }
  };

  if constexpr (RING) {
    // prologue: up to five halves (tiles 0 and 1 and the first half of tile 2)
    if (total > 0) { ring_issue0(); ring_issue1(); }
    if (total > 1) { ring_issue0(); ring_issue1(); }
    if (total > 2) ring_issue0();
  } else {
#pragma unroll
    for (int s = 0; s < NST - 1; ++s)
      if (s < total) issue_next(s);
  }

  // RES 3 (PLAIN): alpha 1, no bias / ReLU / fused sum -- a compile-time epilogue, so the kernel
  // carries one store loop with nothing but the pair exchange, the bf16 packing and the stores;
  // for f32 output: f32 split-K slabs only (no atomics, accumulate, bias, bf16 slabs)
  // RES 4 (BSUM): alpha 1, an f32 bias, no ReLU (the out-projection: bias + fused loss sum)
  constexpr bool PLAIN = RES == 3, BSUM = RES == 4, NOALPHA = PLAIN || BSUM;
  constexpr bool HAS_R = RES == 1 || RES == 2;
  const bool relu = !PLAIN && !BSUM && (p.flags & 1);
  const bool has_bias = BSUM || (!PLAIN && (p.flags & 2) && p.splitk == 1);
  const bool bias_f32 = BSUM || (p.flags & 4);
  const bool accumulate = !PLAIN && (p.flags & 8);
  // flags & 32: output stores with sc1, which drop the written lines from the XCD's L2 (plain
  // stores keep them) so the output stream does not evict the operand panels other blocks reuse
  const bool st_sc1 = p.flags & 32;
  const bool psum_on = !OUT_F32 && !PLAIN && p.psum != nullptr;
  float tsum = 0.f;
  const bool slabs = OUT_F32 && (PLAIN || (p.flags & kSlabs));  // (f32 PLAIN: slab mode only)
  const __amdgpu_buffer_rsrc_t rc = make_rsrc(
      p.C, (OUT_F32 ? 4 : 2) *
               ((long)((slabs ? p.splitk * p.batch : p.batch) - 1) * p.sC + (long)(p.M - 1) * p.ldc + p.N));
  bool after_epi = false;

  // K-tile g landed in LDS for every wave, and every wave's fragment reads of tile g - 1
  // completed (so its stage may be refilled): this wave's pieces of g (the younger tiles' pieces
  // and, right after an epilogue, its S_EPI stores may stay in flight), then the barrier
  auto wait_landed = [&](int g) {
    stamp();
    const bool tail = g + NST - 2 >= total;
    if constexpr (NST >= 3) {
      if (tail) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      else if (SWAP && after_epi && psum_on)
        asm volatile("s_waitcnt vmcnt(%0)" ::"n"(L * (NST - 2) + S_EPI + 1) : "memory");
      else if (SWAP && after_epi) asm volatile("s_waitcnt vmcnt(%0)" ::"n"(L * (NST - 2) + S_EPI) : "memory");
      else asm volatile("s_waitcnt vmcnt(%0)" ::"n"(L * (NST - 2)) : "memory");
    } else {
      if (SWAP && after_epi && psum_on) asm volatile("s_waitcnt vmcnt(%0)" ::"n"(S_EPI + 1) : "memory");
      else if (SWAP && after_epi) asm volatile("s_waitcnt vmcnt(%0)" ::"n"(S_EPI) : "memory");
      else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    }
    after_epi = false;
    stamp();
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();
    stamp();
  };
  // ---- RING schedule (one barrier per K-tile, as before; what changes is what is in flight).
  //   prologue        halves 0 .. 4                                   (as many as exist)
  //   top of tile f   counted vmcnt: halves 2 f and 2 f + 1 landed;  lgkmcnt(0);  s_barrier
  //   after it        (f >= 1) halves 2 f + 3 and 2 f + 4 into the slots of tile f - 1's halves
  //                   2 f - 2 and 2 f - 1, which every wave finished reading (lgkmcnt(0)) before
  //                   it entered this barrier; the other three slots hold 2 f, 2 f + 1 (read now)
  //                   and 2 f + 2 (in flight)
  //   then            k-step 0 from half 2 f's slot, k-step 1 from half 2 f + 1's: the fragments
  //                   and, per output element, the MFMA order of the two-stage loop (the reads
  //                   themselves are the tr_read* statements: see there)
  // So half 2 f + 2 is asked for two K-tiles before its wait and half 2 f + 3 one K-tile before
  // (the two-stage loop: about one and about one half), and a tile's reads come one barrier after
  // the wait that retired its halves, never in the same phase.
  // The count.  Halves are issued in order and vmcnt retires in order, so "halves 2 f, 2 f + 1
  // landed" is vmcnt(4 n + e) with n = the halves issued after 2 f + 1 so far and e = the younger
  // non-DMA entries of the queue.  Before the top of tile f the halves issued are 0 .. 4 (f = 0)
  // or 0 .. 2 f + 2 (f >= 1), cut off at the sequence's last half 2 total - 1:
  //   f = 0:  n = 3, or 2 total - 2 when total <= 2 (nk = 1 or 2 on a one-item block: 0 or 2 -- the
  //           ring never wraps, every half has its own slot);
  //   f >= 1: n = 1, or 0 on the last tile (the tail: nothing left to issue, so the last tile
  //           waits vmcnt(0)).  Inside the loop of a longer sequence the count is never 0.
  // Item change (a persistent block): the sequence is flat, so the halves above are the NEXT item's
  // and stay in flight across the epilogue; f >= 1 there.  The epilogue's stores are younger than
  // every half issued so far: with one 16-byte buffer store per accumulator block from every lane
  // (rows / columns past M / N leave through an out-of-range offset, as in the bf16 kernels) they
  // are exactly e = E_RING entries.  When the stores are not that uniform (unaligned C, N % 4) e
  // stays 0: a count that is too small only waits for more.  A timeline stamp before the wait is
  // one more entry.  The block's last item is followed by nothing: its tile waited vmcnt(0) and
  // passed a barrier, which is what staging the slab through the (whole) ring needs.
  int ring_epi = 0;   // E_RING when the previous item's stores were counted
  auto ring_wait = [&](int f) {
    const int st = stamp_st();
    const int n = f == 0 ? (total > 2 ? 3 : 2 * total - 2) : (f + 1 < total ? 1 : 0);
    if (n == 1 && !ring_epi) {   // steady state
      if (st) asm volatile("s_waitcnt vmcnt(5)" ::: "memory");
      else asm volatile("s_waitcnt vmcnt(4)" ::: "memory");
    } else {
      wait_vm_n(4 * n + ring_epi + st);
    }
    ring_epi = 0;
    stamp();
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();
    stamp();
  };
  // Software-pipelined by half a K-tile: the fragments of k-step 0 of tile g + 1 are read (and
  // tile g + 1's barrier passed) while the k-step 1 MFMAs of tile g are still to issue, so the
  // MFMA pipe never waits for a barrier plus an LDS round trip at a tile boundary (it did, once
  // per K-tile per wave).  ka/kb: k-step 0 fragments, la/lb: k-step 1.
  bf16x8 ka[TM], kb[TN], la[TM], lb[TN];
  auto read_frags = [&](int g, int ks, bf16x8* af, bf16x8* bfr) {
    const bf16_t* As_ = smem + (g % NST) * STAGE;
    const bf16_t* Bs_ = As_ + A_TILE;
#pragma unroll
    for (int ii = 0; ii < TM; ++ii) af[ii] = frag<BM, A_KC>(As_, wr * (BM / WM) + ii * 16, ks, lane);
#pragma unroll
    for (int j = 0; j < TN; ++j) bfr[j] = frag<BN, B_KC>(Bs_, wc * (BN / WN) + j * 16, ks, lane);
  };
  auto mfmas = [&](const bf16x8* af, const bf16x8* bfr) {
#pragma unroll
    for (int ii = 0; ii < TM; ++ii)
#pragma unroll
      for (int j = 0; j < TN; ++j) {
        if constexpr (SWAP) acc[ii][j] = mfma16x16x32(bfr[j], af[ii], acc[ii][j]);  // C^T block
        else acc[ii][j] = mfma16x16x32(af[ii], bfr[j], acc[ii][j]);
      }
  };
  static_assert(BK == 64, "two k-steps per K-tile");
  // LJS_GEMM_PIN (off: neutral at B=64, +0.7 us on the 8-wave 128x128 QKV at B=8, gpurun_out/r4p):
  // the k-step 1 fragments (la / lb) are redefined through an empty asm right after
  // the k-step 0 MFMAs (a sched_barrier keeps it there).  The compiler then places its lgkmcnt
  // wait for them at that point, where their reads are long done, instead of in front of the
  // k-step 1 MFMAs -- where, with the next tile's fragment reads issued after the barrier still
  // in flight (and an SMEM load on the item-change path), it could only emit lgkmcnt(0) and so
  // exposed the new reads' LDS latency once per K-tile.
#ifndef LJS_GEMM_PIN
#define LJS_GEMM_PIN 0
#endif
  auto pin = [&](bf16x8* af, bf16x8* bfr) {
#if LJS_GEMM_PIN
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int ii = 0; ii < TM; ++ii) asm volatile("" : "+v"(af[ii]));
#pragma unroll
    for (int j = 0; j < TN; ++j) asm volatile("" : "+v"(bfr[j]));
#endif
  };
  // (wave tiles with more than 8 fragments per k-step -- 128x160's 32x160 -- keep the plain
  // loop: two fragment sets would not fit beside their epilogue registers; so do the
  // transposed-read weight-gradient kernels, 1-2 % slower pipelined while the k-contiguous
  // forward / dX kernels gain 3-4 %: QKV 2561 45.3 -> 43.7 us, 1282 48.1 -> 46.1 us)
  // (one 8-wave block per CU has 256 VGPRs per wave: 10 fragments fit twice beside 24 accumulators)
  // (one 4-wave block per CU -- the wide wave tiles 128x64 .. 128x128 -- has 512 registers per
  // wave: both fragment sets fit beside up to 256 accumulators)
  constexpr bool ONE_PER_CU = !(NW == 4 && NST * (BM + BN) * 64 * 2 <= 80 * 1024);
  constexpr bool PIPE = (TM + TN <= 8 || (NW == 8 && TM + TN <= 10) || (NW == 4 && ONE_PER_CU && TM + TN <= 16)) &&
                        A_KC && B_KC;   // (the last clause: 4-wave wide wave tiles, none instantiated since r5b)
  if (PIPE && total > 0) {
    wait_landed(0);
    read_frags(0, 0, ka, kb);
    if (NST - 1 < total) issue_next((NST - 1) % NST);
  }

  for (int it = 0, f = 0; it < my_items; ++it) {
  for (int kk = 0; kk < nk; ++kk, ++f) {
    if constexpr (RING) {
      const bf16_t* h0 = smem + ring_r;
      const bf16_t* h1 = smem + ring_adv(ring_r, 1);
      ring_r = ring_adv(ring_r, 2);
      // fragment reads as asm statements (tr_read*: the compiler must not see them, or it drains
      // the ring).  Raw halves r[0] = A row block 0, r[1..4] = B column blocks 0..3 -- what the
      // first four MFMAs need, valid when tr_read5_wait ends -- and r[5..7] = A row blocks 1..3,
      // in flight until tr_wait3_8 below.
      auto addr_half = [&](const bf16_t* hs, unsigned* ad) {
        ad[0] = frag_tr_addr(hs, wr * (BM / WM), lane);
#pragma unroll
        for (int j = 0; j < TN; ++j) ad[1 + j] = frag_tr_addr(hs + A_HALF, wc * (BN / WN) + j * 16, lane);
#pragma unroll
        for (int ii = 1; ii < TM; ++ii) ad[4 + ii] = frag_tr_addr(hs, wr * (BM / WM) + ii * 16, lane);
      };
      auto row0 = [&](const s16x4* lo, const s16x4* hi) {
        const bf16x8 a0 = join_bf16x8(lo[0], hi[0]);
#pragma unroll
        for (int j = 0; j < TN; ++j) acc[0][j] = mfma16x16x32(join_bf16x8(lo[1 + j], hi[1 + j]), a0, acc[0][j]);
      };
      auto rows123 = [&](const s16x4* lo, const s16x4* hi) {
#pragma unroll
        for (int ii = 1; ii < TM; ++ii) {
          const bf16x8 a = join_bf16x8(lo[4 + ii], hi[4 + ii]);
#pragma unroll
          for (int j = 0; j < TN; ++j) acc[ii][j] = mfma16x16x32(join_bf16x8(lo[1 + j], hi[1 + j]), a, acc[ii][j]);
        }
      };
      static_assert(TM == 4 && TN == 4 && SWAP, "the tr_read* groups are written for 4 x 4 fragments");
      unsigned ad0[8], ad1[8];
      s16x4 r0lo[8], r0hi[8], r1lo[8], r1hi[8];
      addr_half(h0, ad0);
      addr_half(h1, ad1);
      ring_wait(f);
      tr_read5_wait(r0lo, r0hi, ad0);                    // k-step 0: A 0, B 0..3
      tr_read3(r0lo + 5, r0hi + 5, ad0 + 5);             // k-step 0: A 1..3
      tr_read4(r1lo, r1hi, ad1);                         // k-step 1: A 0, B 0..2
      tr_read4(r1lo + 4, r1hi + 4, ad1 + 4);             // k-step 1: B 3, A 1..3
      if (f >= 1 && f + 1 < total) ring_issue1();        // half 2 f + 3 into half 2 f - 2's slot
      if (f >= 1 && f + 2 < total) ring_issue0();        // half 2 f + 4 into half 2 f - 1's slot
      row0(r0lo, r0hi);
      tr_wait3_8(r0lo + 5, r0hi + 5, r1lo, r1hi);        // (long landed: the issues above took longer)
      rows123(r0lo, r0hi);
      row0(r1lo, r1hi);
      rows123(r1lo, r1hi);
      continue;
    }
    if constexpr (!PIPE) {
      // barrier for tile f, then per k-step: fragment reads, half of tile f + NST - 1's DMA
      // pieces (their issue time overlaps the LDS latency), MFMAs
      wait_landed(f);
      const bool more = f + NST - 1 < total;
      const int nst = (f + NST - 1) % NST;
      read_frags(f, 0, ka, kb);
      if (more) issue_half(nst, false);
      mfmas(ka, kb);
      read_frags(f, 1, la, lb);
      if (more) issue_half(nst, true);
      mfmas(la, lb);
      continue;
    }
    read_frags(f, 1, la, lb);
    mfmas(ka, kb);
    pin(la, lb);
    // inside an item: DMA of tile f + NST into the stage of tile f (free once barrier f + 1 is
    // passed), issued in two halves around the k-step 1 MFMAs.  An item's last tile does this
    // after its epilogue instead (below), so no fragments are live across the epilogue.
    const bool inner = kk + 1 < nk;
    const bool more = inner && f + NST < total;
    if (inner) {
      wait_landed(f + 1);
      read_frags(f + 1, 0, ka, kb);
      if (more) issue_half(f % NST, false);
    }
    mfmas(la, lb);
    if (more) issue_half(f % NST, true);
  }

    // ------------------------------------------------------------ epilogue of this item
    const WorkItem w = decode_item(p, slot + G * it, ntm, ntn);
    const int m0 = w.m0 * BM + wr * (BM / WM), n0 = w.n0 * BN + wc * (BN / WN);
    const int g = lane >> 4;
    if constexpr (!OUT_F32) {
#include "gemm_epi_bf16.h"   // S_EPI (+1 fused-sum) stores per lane: what wait_landed counts after_epi
      after_epi = true;
    } else {
      // lane holds C[16 ii + (lane & 15)][16 j + 4 g + 0..3]
      const bool vec = (p.ldc & 3) == 0 && (p.sC & 3) == 0 && ((((uintptr_t)p.C) & 15) == 0);
      [[maybe_unused]] const bool ring_exact = RING && vec && (p.N & 3) == 0;
      if constexpr (BN / WN == 64 && WM * WN * (BM / WM) * 256 <= NST * STAGE * 2) {
        if (slabs && vec && (p.flags & kSlabVst) && it + 1 == my_items && !has_bias && !relu && !accumulate) {
          // no DMA is in flight after the block's last item: once every wave's last fragment reads
          // are done the ring holds this wave's 64-column f32 rows (wave-private image)
          __syncthreads();
          unsigned char* img = reinterpret_cast<unsigned char*>(smem) + wave * (BM / WM) * 256;
#pragma unroll
          for (int ii = 0; ii < TM; ++ii) {
            const int r = ii * 16 + (lane & 15);
#pragma unroll
            for (int j = 0; j < TN; ++j)
              *reinterpret_cast<f32x4*>(img + r * 256 + (((4 * j + g) ^ (r & 7)) << 4)) = PLAIN ? acc[ii][j] : acc[ii][j] * p.alpha;
          }
          asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
          const long cb = (long)(w.split * p.batch + w.b) * p.sC;
#pragma unroll
          for (int q = 0; q < (BM / WM) / 4; ++q) {
            const int r = 4 * q + (lane >> 4), c = lane & 15;
            const f32x4 v = *reinterpret_cast<const f32x4*>(img + r * 256 + ((c ^ (r & 7)) << 4));
            const int row = m0 + r, col = n0 + 4 * c;
            if (row < p.M && col + 4 <= p.N) {
              const u32x4 bits = __builtin_bit_cast(u32x4, v);
              __builtin_amdgcn_raw_buffer_store_b128(bits, rc, (int)((cb + (long)row * p.ldc + col) * 4), 0, 0);
            } else if (row < p.M) {
              float* C = reinterpret_cast<float*>(p.C) + cb + (long)row * p.ldc + col;
#pragma unroll
              for (int e = 0; e < 4; ++e)
                if (col + e < p.N) C[e] = v[e];
            }
          }
          continue;  // the block's last item: nothing follows
        }
      }
      // this item's output block (slab mode: slab (split, batch b) = split * batch + b, so the
      // slabs of a batch of weight gradients are [S][batch][M][N]: one slab_reduce combines all)
      const long cb = (long)(slabs ? w.split * p.batch + w.b : w.b) * p.sC;
#pragma unroll
      for (int j = 0; j < TN; ++j) {
        const int col = n0 + j * 16 + 4 * g;
        float bv[4] = {0.f, 0.f, 0.f, 0.f};
        if (has_bias) {
#pragma unroll
          for (int e = 0; e < 4; ++e) {
            if (col + e >= p.N) continue;
            const long bo = (long)w.b * p.sBias + col + e;
            bv[e] = bias_f32 ? reinterpret_cast<const float*>(p.bias)[bo]
                             : bf2f(reinterpret_cast<const bf16_t*>(p.bias)[bo]);
          }
        }
#pragma unroll
        for (int ii = 0; ii < TM; ++ii) {
          const int row = m0 + ii * 16 + (lane & 15);
          f32x4 v;
#pragma unroll
          for (int e = 0; e < 4; ++e) {
            v[e] = PLAIN ? acc[ii][j][e] : acc[ii][j][e] * p.alpha + bv[e];
            if (relu) v[e] = fmaxf(v[e], 0.f);
          }
          acc[ii][j] = f32x4{0.f, 0.f, 0.f, 0.f};
          if constexpr (RING) {
            if (ring_exact) {   // every lane stores: the next wait counts these E_RING entries
              const bool ok = row < p.M && col < p.N;   // N % 4 == 0: chunks are whole
              const int off = ok ? (int)((cb + (long)row * p.ldc + col) * 4) : 0x7ffffff0;
              const u32x4 bits = __builtin_bit_cast(u32x4, v);
              if (st_sc1) __builtin_amdgcn_raw_buffer_store_b128(bits, rc, off, 0, kSC1);
              else __builtin_amdgcn_raw_buffer_store_b128(bits, rc, off, 0, 0);
              continue;
            }
          }
          if (row >= p.M || col >= p.N) continue;
          float* C = reinterpret_cast<float*>(p.C) + cb + (long)row * p.ldc + col;
          if (p.splitk > 1 && !slabs) {
#pragma unroll
            for (int e = 0; e < 4; ++e)
              if (col + e < p.N) atomicAdd(C + e, v[e]);
          } else if (vec && col + 4 <= p.N) {
            if (accumulate) v += *reinterpret_cast<const f32x4*>(C);
            const int off = (int)((cb + (long)row * p.ldc + col) * 4);
            const u32x4 bits = __builtin_bit_cast(u32x4, v);
            if (st_sc1) __builtin_amdgcn_raw_buffer_store_b128(bits, rc, off, 0, kSC1);
            else __builtin_amdgcn_raw_buffer_store_b128(bits, rc, off, 0, 0);
          } else {
#pragma unroll
            for (int e = 0; e < 4; ++e)
              if (col + e < p.N) C[e] = accumulate ? C[e] + v[e] : v[e];
          }
        }
      }
      // drain before the next item's counted waits; after the block's last item the wave just
      // ends (its stores complete on their own and the CU is free for the next block sooner)
      // (RING: no drain -- the next item's halves are in flight and the next wait counts the stores)
      if constexpr (RING) ring_epi = ring_exact ? E_RING : 0;
      else if (it + 1 < my_items) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    }
    // the next item's first tile (f): its barrier, k-step 0 fragments and the DMA of tile
    // f + NST - 1 (the stage of tile f - 1, read by every wave before this barrier)
    if (PIPE && f < total) {
      wait_landed(f);
      read_frags(f, 0, ka, kb);
      if (f + NST - 1 < total) issue_next((f + NST - 1) % NST);
    }
  }
  stamp_end();
}

template <int BM, int BN, int WM, int WN, int NST, bool A_KC, bool B_KC, bool OUT_F32, int RES = 0>
__global__ __launch_bounds__(WM * WN * 64, (WM * WN == 4 && NST * (BM + BN) * 64 * 2 <= 80 * 1024) ? 2 : 1) void
gemm_dma_kernel(GemmArgs p) {
  gemm_dma_body<BM, BN, WM, WN, NST, A_KC, B_KC, OUT_F32, RES>(p, blockIdx.x, gridDim.x);
}

// Two GEMMs of the same kernel instance in ONE grid, one block per work item: blocks [0, g0) take
// p0's items, the rest p1's.  The weight-gradient GEMMs of a layer at the reference shape (dW_qkv
// and dW_o, 240 short items each) are latency-bound launches; grouped they share one round of
// resident blocks instead of running back to back (ops/linear.py dW grouping).
template <int BM, int BN, int WM, int WN, int NST, bool A_KC, bool B_KC, bool OUT_F32, int RES = 0>
__global__ __launch_bounds__(WM * WN * 64, (WM * WN == 4 && NST * (BM + BN) * 64 * 2 <= 80 * 1024) ? 2 : 1) void
gemm_dma_group2_kernel(GemmArgs p0, GemmArgs p1, int g0) {
  if ((int)blockIdx.x < g0)
    gemm_dma_body<BM, BN, WM, WN, NST, A_KC, B_KC, OUT_F32, RES>(p0, blockIdx.x, g0);
  else
    gemm_dma_body<BM, BN, WM, WN, NST, A_KC, B_KC, OUT_F32, RES>(p1, blockIdx.x - g0, gridDim.x - g0);
}

// ============================================================================ lean K-loop GEMM
// The persistent LDS-DMA GEMM's k-contiguous, bf16-output path (forward projections and dX GEMMs)
// with the per-K-tile bookkeeping out of the K-loop.  A DMA / MFMA / barrier probe
// (scripts/probe_dma_mfma.hip, profiles/r5_probe_dma_mfma.txt) measured what a K-tile of this
// structure costs per SIMD: 32 MFMAs per wave alone 1180 cycles; + 6 DMA pieces and 16 fragment
// reads + one barrier 1440; + ~90 scalar instructions and 6 branches per K-tile 1850 -- and the
// general kernel above carries about that much (stage index = tile mod NST through mul_hi, the
// tail / after-epilogue / next-item tests and their vmcnt selection, all inside the loop).  Here:
//  * the stage is a rotating offset (the DMA of tile f + NST goes to tile f's stage);
//  * the K-loop of an item runs nk - 1 identical steps (one counted vmcnt, one barrier, half
//    the next tile's pieces after its k-step-0 fragment reads, half after the k-step-1 MFMAs); the
//    item's last K-tile, its epilogue and the next item's first barrier are peeled;
//  * the issue cursor never tests for the end: past the block's last item it issues K-tiles that
//    read zeros (an empty-range descriptor) into stages nothing reads again, so every step's count is the same.
// Operands, images, fragment reads and MFMA orientation are gemm_dma_kernel's; the epilogue is
// shared with it, one text included by both (gemm_epi_bf16.h)
// (bit-identical results: tests/test_kernels_gpu.py::test_gemm_lean_bit_exact).
// The issue cursor's K-tiles past the block's last item go through a buffer descriptor with an
// empty range: every lane is out of range whatever its offsets, so the pieces read zeros without a
// memory access and retire at once (the block's final vmcnt(0) does not wait for an L2 round trip).
template <int BM, int BN, int WM, int WN, int NST, int RES>
__global__ __launch_bounds__(WM * WN * 64, (WM * WN == 4 && NST * (BM + BN) * 64 * 2 <= 80 * 1024) ? 2 : 1) void
gemm_lean_kernel(GemmArgs p) {
  constexpr int NW = WM * WN;
  constexpr int TM = BM / WM / 16, TN = BN / WN / 16;
  constexpr int A_TILE = BM * BK, B_TILE = BN * BK, STAGE = A_TILE + B_TILE;
  using TA = DmaTile<BM, true, NW>;
  using TB = DmaTile<BN, true, NW>;
  constexpr int L = TA::PER_WAVE + TB::PER_WAVE;
  static_assert(TN % 2 == 0, "column blocks pair up for 16-byte stores");
  static_assert(NST >= 2, "at least one K-tile in flight");
  constexpr int S_EPI = TM * TN / 2;
  static_assert(L * (NST - 1) + S_EPI + 1 <= 63, "vmcnt immediate range");
  constexpr bool PLAIN = RES == 3, BSUM = RES == 4, NOALPHA = PLAIN || BSUM;
  constexpr bool HAS_R = RES == 1 || RES == 2;
  __shared__ __attribute__((aligned(16))) bf16_t smem[NST * STAGE];

  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wr = wave / WN, wc = wave % WN;
  const int ntm = (p.M + BM - 1) / BM, ntn = (p.N + BN - 1) / BN;
  const int items = p.batch * ntm * ntn;
  const int G = gridDim.x;
  const int slot = xcd_remap(blockIdx.x, G);
  const int my_items = slot < items ? (items - slot + G - 1) / G : 0;
  if (my_items == 0) return;
  const int nk = p.kt_per_split;   // K / 64 (no split-K on this path)

  const long a_bytes = 2 * ((long)(p.M - 1) * p.lda + p.K);
  const long b_bytes = 2 * ((long)(p.N - 1) * p.ldb + p.K);
  TA ta;
  TB tb;
  ta.init(p.lda, wave, lane);
  tb.init(p.ldb, wave, lane);

  // ---- issue cursor: the item whose K-tiles are being fetched (NST K-tiles ahead of the MFMAs)
  int is_item = 0, is_kt = 0;
  __amdgpu_buffer_rsrc_t ra, rb;
  int a_off = 0, b_off = 0;
  auto load_item = [&](int k) {
    const WorkItem w = decode_item(p, slot + G * (k < my_items ? k : 0), ntm, ntn);
    ra = make_rsrc(p.A + (long)w.b * p.sA, a_bytes);
    rb = make_rsrc(p.B + (long)w.b * p.sB, b_bytes);
    a_off = __builtin_amdgcn_readfirstlane((int)((long)w.m0 * BM * p.lda * 2));
    b_off = __builtin_amdgcn_readfirstlane((int)((long)w.n0 * BN * p.ldb * 2));
    if (k >= my_items) {   // past the block's last item: an empty range (every piece reads zeros)
      ra = make_rsrc(p.A, 0);
      rb = make_rsrc(p.B, 0);
    }
  };
  auto issue_a = [&](int so) { ta.issue(ra, smem + so, a_off, wave); };
  auto issue_b = [&](int so) { tb.issue(rb, smem + so + A_TILE, b_off, wave); };
  auto advance = [&]() {
    a_off += BK * 2;
    b_off += BK * 2;
    if (++is_kt == nk) {
      is_kt = 0;
      load_item(++is_item);
    }
  };

  f32x4 acc[TM][TN];
#pragma unroll
  for (int i = 0; i < TM; ++i)
#pragma unroll
    for (int j = 0; j < TN; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};

  load_item(0);
#pragma unroll
  for (int s = 0; s < NST - 1; ++s) {
    issue_a(s * STAGE);
    issue_b(s * STAGE);
    advance();
  }

  const bool relu = !PLAIN && !BSUM && (p.flags & 1);
  const bool has_bias = BSUM || (!PLAIN && (p.flags & 2));
  const bool bias_f32 = BSUM || (p.flags & 4);
  const bool st_sc1 = p.flags & 32;
  const bool psum_on = !PLAIN && p.psum != nullptr;
  const __amdgpu_buffer_rsrc_t rc = make_rsrc(p.C, 2 * ((long)(p.batch - 1) * p.sC + (long)(p.M - 1) * p.ldc + p.N));

  bf16x8 ka[TM], kb[TN], la[TM], lb[TN];
  auto read_frags = [&](int so, int ks, bf16x8* af, bf16x8* bfr) {
    const bf16_t* As_ = smem + so;
    const bf16_t* Bs_ = As_ + A_TILE;
#pragma unroll
    for (int ii = 0; ii < TM; ++ii) af[ii] = frag<BM, true>(As_, wr * (BM / WM) + ii * 16, ks, lane);
#pragma unroll
    for (int j = 0; j < TN; ++j) bfr[j] = frag<BN, true>(Bs_, wc * (BN / WN) + j * 16, ks, lane);
  };
  auto mfmas = [&](const bf16x8* af, const bf16x8* bfr) {
#pragma unroll
    for (int ii = 0; ii < TM; ++ii)
#pragma unroll
      for (int j = 0; j < TN; ++j) acc[ii][j] = mfma16x16x32(bfr[j], af[ii], acc[ii][j]);  // C^T block
  };
  auto next_so = [](int so) { return so + STAGE == NST * STAGE ? 0 : so + STAGE; };
  auto barrier = []() {
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();
  };

  // the stage of the (virtual) tile before the block's first: the first item start issues the
  // DMA of tile NST - 1 into it
  int so = (NST - 1) * STAGE;
  // item start: tile f = the item's first (stage nso) landed -- this wave's pieces of the younger
  // tiles and, after an epilogue, its S_EPI (+1 fused-sum) stores may stay in flight -- then the
  // barrier, k-step 0 fragments, and the DMA of tile f + NST - 1 into the stage of tile f - 1
  auto item_start = [&](bool after_epi) {
    if (!after_epi) asm volatile("s_waitcnt vmcnt(%0)" ::"n"(L * (NST - 2)) : "memory");
    else if (psum_on) asm volatile("s_waitcnt vmcnt(%0)" ::"n"(L * (NST - 2) + S_EPI + 1) : "memory");
    else asm volatile("s_waitcnt vmcnt(%0)" ::"n"(L * (NST - 2) + S_EPI) : "memory");
    barrier();
    const int nso = next_so(so);
    read_frags(nso, 0, ka, kb);
    issue_a(so);
    issue_b(so);
    advance();
    so = nso;
  };
  item_start(false);

  float tsum = 0.f;
  for (int it = 0; it < my_items; ++it) {
    for (int kk = 0; kk + 1 < nk; ++kk) {
      read_frags(so, 1, la, lb);
      mfmas(ka, kb);
      const int nso = next_so(so);
      asm volatile("s_waitcnt vmcnt(%0)" ::"n"(L * (NST - 2)) : "memory");  // tile f + 1 landed
      barrier();                                   // ... for every wave; every read of tile f done
      read_frags(nso, 0, ka, kb);
      issue_a(so);                                 // tile f + NST into tile f's stage
      mfmas(la, lb);
      issue_b(so);
      advance();
      so = nso;
    }
    // the item's last K-tile
    read_frags(so, 1, la, lb);
    mfmas(ka, kb);
    mfmas(la, lb);

    // ------------------------------------------------------------ epilogue of this item
    const WorkItem w = decode_item(p, slot + G * it, ntm, ntn);
    const int m0 = w.m0 * BM + wr * (BM / WM), n0 = w.n0 * BN + wc * (BN / WN);
    const int g = lane >> 4;
#include "gemm_epi_bf16.h"   // S_EPI (+1 fused-sum) stores per lane: what item_start(true) counts
    if (it + 1 < my_items) item_start(true);
  }
  // the DMA pieces still in flight (the cursor's past-the-end tiles) write this block's LDS: let
  // them finish before the block's LDS can be handed to another
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
}


// ============================================================================ host side
// The LDS-DMA tile table: everything a tile code stands for, stated once.  The explicit
// instantiations, the instance names, the dispatch, the demotion chain and the psum geometry
// below all come from these lines.
//   code, BM x BN block tile, WM x WN waves, NST ring stages, then what the tile has:
//   KK    k-contiguous operands, bf16 output: 0 nothing; 1 the RES 0 instance; 5 the epilogue
//         instances RES 0-4; 3 the same five instantiated, but a call with an epilogue operand
//         (RES 1 / 2) demotes the tile
//   KKF   k-contiguous operands, f32 output
//   MIX   the other five layout / output pairs (one operand m/n-contiguous, or both with bf16 output)
//   MN    m/n-contiguous operands, f32 output (weight gradients): 1 the RES 0 instance; 2 also
//         the plain split-K slab instance (RES 3) and the grouped-pair kernel
//   LEAN  a lean K-loop twin of the KK instances: 1 only when forced (code + 100000: the general
//         kernel measured 14.4 vs 14.8 us at 128x160, one item per block), 2 by default
//   DEMOTE  the code a call falls to when the tile has no instance for it, or the operands do not
//         meet the LDS-DMA kernels' conditions; every chain ends at a register-staged tile
//   UNFOLD  0: batches run as they are; else the tile runs a batch only folded into one GEMM
//         over N * batch columns, and this is the code of a batch that cannot be folded
// 64x64: the small-M GEMMs of the reference shape (2048 tokens), where 128x128 tiles leave most
// CUs idle.  128x160 (4 waves stacked along M): N = 640 is 4 column tiles, so a [16384, 640]
// output is exactly one round of 2 blocks/CU.  256x192 (8 waves of 64x96, 112 KiB): 7 DMA pieces
// and 20 fragment reads per wave per 48 MFMAs (256x128: 6 and 16 per 32).  256x128 / 128x256
// weight-gradient tiles: 48 KiB of operands per K-tile for twice the MFMA work of 128x128.
// 128x128 with 8 waves (2 x 4): two waves per SIMD at one block per CU, so a deep ring does not
// cost MFMA/LDS overlap.
#define LJS_GEMM_TILES(X)                                       \
  /* code    BM   BN  WM WN NST KK KKF MIX MN LEAN DEMOTE UNFOLD */ \
  X(643,     64,  64, 2, 2, 3,  1, 1,  1,  1, 0,   64,    0)    \
  X(644,     64,  64, 2, 2, 4,  3, 1,  1,  1, 2,   64,    0)    \
  X(1282,   128, 128, 2, 2, 2,  5, 1,  1,  2, 2,   128,   0)    \
  X(1284,   128, 128, 2, 2, 4,  5, 1,  1,  1, 2,   128,   0)    \
  X(1602,   128, 160, 4, 1, 2,  5, 0,  0,  0, 1,   1282,  0)    \
  X(2561,   256, 128, 4, 2, 3,  5, 1,  0,  0, 2,   1284,  0)    \
  X(2562,   256, 192, 4, 2, 2,  3, 0,  0,  0, 2,   1282,  2561) \
  X(2563,   256, 128, 4, 2, 3,  0, 0,  0,  1, 0,   1282,  0)    \
  X(12856,  128, 256, 2, 4, 3,  0, 0,  0,  1, 0,   1282,  0)    \
  X(12883,  128, 128, 2, 4, 3,  5, 1,  0,  2, 2,   1282,  0)    \
  X(12884,  128, 128, 2, 4, 4,  5, 1,  0,  2, 2,   1282,  0)
// code + kForceLean runs a tile's lean K-loop kernel where it has one, + 2 * kForceLean the
// general one (A/B timing and the bit-exact tests)
constexpr int kForceLean = 100000;

// explicit instantiations: hipcc (ROCm 7.2) otherwise leaves some of these kernels' host stubs
// undefined when they are only named inside the dispatch's templates
#define LJS_DMA_INST(BM, BN, WM, WN, NST, AK, BKc, OF, RES) \
  template __global__ void gemm_dma_kernel<BM, BN, WM, WN, NST, AK, BKc, OF, RES>(GemmArgs);
#define LJS_LEAN_INST(BM, BN, WM, WN, NST, RES) \
  template __global__ void gemm_lean_kernel<BM, BN, WM, WN, NST, RES>(GemmArgs);
#define LJS_INST_KK_0(...)
#define LJS_INST_KK_1(...) LJS_DMA_INST(__VA_ARGS__, true, true, false, 0)
#define LJS_INST_KK_5(...)                                                                 \
  LJS_INST_KK_1(__VA_ARGS__) LJS_DMA_INST(__VA_ARGS__, true, true, false, 1)               \
  LJS_DMA_INST(__VA_ARGS__, true, true, false, 2) LJS_DMA_INST(__VA_ARGS__, true, true, false, 3) \
  LJS_DMA_INST(__VA_ARGS__, true, true, false, 4)
#define LJS_INST_KK_3(...) LJS_INST_KK_5(__VA_ARGS__)
#define LJS_INST_KKF_0(...)
#define LJS_INST_KKF_1(...) LJS_DMA_INST(__VA_ARGS__, true, true, true, 0)
#define LJS_INST_MIX_0(...)
#define LJS_INST_MIX_1(...)                                                                      \
  LJS_DMA_INST(__VA_ARGS__, false, false, false, 0) LJS_DMA_INST(__VA_ARGS__, true, false, false, 0) \
  LJS_DMA_INST(__VA_ARGS__, true, false, true, 0) LJS_DMA_INST(__VA_ARGS__, false, true, false, 0)   \
  LJS_DMA_INST(__VA_ARGS__, false, true, true, 0)
#define LJS_INST_MN_0(...)
#define LJS_INST_MN_1(...) LJS_DMA_INST(__VA_ARGS__, false, false, true, 0)
#define LJS_INST_MN_2(...)                                                          \
  LJS_INST_MN_1(__VA_ARGS__) LJS_DMA_INST(__VA_ARGS__, false, false, true, 3)       \
  template __global__ void gemm_dma_group2_kernel<__VA_ARGS__, false, false, true, 3>(GemmArgs, GemmArgs, int);
#define LJS_INST_LEAN_0(...)
#define LJS_INST_LEAN_1(...)                                                                        \
  LJS_LEAN_INST(__VA_ARGS__, 0) LJS_LEAN_INST(__VA_ARGS__, 1) LJS_LEAN_INST(__VA_ARGS__, 2)         \
  LJS_LEAN_INST(__VA_ARGS__, 3) LJS_LEAN_INST(__VA_ARGS__, 4)
#define LJS_INST_LEAN_2(...) LJS_INST_LEAN_1(__VA_ARGS__)
#define LJS_INST_TILE(CODE, BM, BN, WM, WN, NST, KK, KKF, MIX, MN, LEAN, DEMOTE, UNFOLD)        \
  LJS_INST_KK_##KK(BM, BN, WM, WN, NST) LJS_INST_KKF_##KKF(BM, BN, WM, WN, NST)                  \
  LJS_INST_MIX_##MIX(BM, BN, WM, WN, NST) LJS_INST_MN_##MN(BM, BN, WM, WN, NST)                  \
  LJS_INST_LEAN_##LEAN(BM, BN, WM, WN, NST)
LJS_GEMM_TILES(LJS_INST_TILE)
#undef LJS_INST_TILE
#undef LJS_LEAN_INST
#undef LJS_DMA_INST

unsigned long long* g_gemm_trace = nullptr;  // LJS_GEMM_TRACE builds: the next LDS-DMA launches' stamps

// instance names, formatted once per instantiation: "gemm_dma<128,128,2,2,4,kc,kc,bf16>"
struct LaunchName { char s[64]; };
#define LJS_NAME_ONCE(...)                  \
  static const LaunchName n = [] {          \
    LaunchName x;                           \
    snprintf(x.s, sizeof x.s, __VA_ARGS__); \
    return x;                               \
  }();                                      \
  return n.s;
template <int BM, int BN, int WM, int WN, int NST, bool AK, bool BKc, bool OF, bool GROUP2>
const char* dma_name() {
  LJS_NAME_ONCE("%s<%d,%d,%d,%d,%d,%s,%s,%s>", GROUP2 ? "gemm_dma_group2" : "gemm_dma", BM, BN, WM, WN, NST,
                AK ? "kc" : "mn", BKc ? "kc" : "mn", OF ? "f32" : "bf16")
}
template <int BM, int BN, int WM, int WN, int NST>
const char* lean_name() {
  LJS_NAME_ONCE("gemm_lean<%d,%d,%d,%d,%d>", BM, BN, WM, WN, NST)
}
template <int BM, int BN, bool AK, bool BKc, bool OF>
const char* reg_name() {
  LJS_NAME_ONCE("gemm_bf16<%d,%d,%s,%s,%s>", BM, BN, AK ? "kc" : "mn", BKc ? "kc" : "mn", OF ? "f32" : "bf16")
}
#undef LJS_NAME_ONCE

// ---------------------------------------------------------------------------- plan
// What one ljs_gemm_bf16 call launches, worked out from the call's numbers alone: gemm_plan
// dereferences nothing and calls no HIP function, so it answers on a machine without a GPU too
// (ljs_gemm_plan).
enum GemmFamily { kFamReg = 0, kFamDma = 1, kFamLean = 2, kFamSlab = 3 };  // kFamSlab: a groupable plain slab GEMM
using GemmKernel = void (*)(GemmArgs);
using GemmGroup2 = void (*)(GemmArgs, GemmArgs, int);

struct GemmPlan {
  hipError_t err;
  int tile;                         // the resolved tile code
  int family;
  int BM, BN, WM, WN, NST;          // the instance (register-staged: 4 waves, 2 buffers)
  bool a_kc, b_kc, out_f32;
  int variant;                      // RES of the LDS-DMA / lean instance, else -1
  int splitk, kt_per_split;
  int N, batch;                     // as launched: a folded batch is one GEMM over N * batch columns
  int items;                        // LDS-DMA / lean work items (tiles x batch x splits)
  unsigned gx, gy, block;
  bool psum, mfast;                 // the kernel writes the fused output sums; kMFast item order
  int psum_count;
  const char* name;
  GemmKernel kernel;
  GemmGroup2 group2;                // kFamSlab: the grouped-pair kernel of the same instance
  const char* group2_name;
};

template <int BM, int BN, int WM, int WN, int NST, bool AK, bool BKc, bool OF, int RES = 0>
void set_dma(GemmPlan& p) {
  p.family = kFamDma;
  p.variant = RES;
  p.kernel = gemm_dma_kernel<BM, BN, WM, WN, NST, AK, BKc, OF, RES>;
  p.name = dma_name<BM, BN, WM, WN, NST, AK, BKc, OF, false>();
}

// the epilogue instance of a k-contiguous bf16-output call, general and lean kernel alike (bf16
// outputs never split)
inline int epilogue_variant(const GemmArgs& a, bool psum) {
  if (a.flags & (kResAdd | kResMask)) return (a.flags & kResF32) ? 2 : 1;
  // plain epilogue (RES 3: compile-time instance, PERF_NOTES r4 "plain instance")
  if (a.alpha == 1.f && !(a.flags & 3) && !psum) return 3;
  // bias (f32) + optional fused sum, alpha 1, no ReLU (RES 4)
  if (a.alpha == 1.f && (a.flags & 7) == 6) return 4;
  return 0;
}

#define LJS_BY_RES(v, X) \
  switch (v) { case 1: X(1); break; case 2: X(2); break; case 3: X(3); break; case 4: X(4); break; default: X(0); }
#define LJS_SET_LEAN(RES) p.kernel = gemm_lean_kernel<BM, BN, WM, WN, NST, RES>
#define LJS_SET_DMA(RES) set_dma<BM, BN, WM, WN, NST, true, true, false, RES>(p)
// The tile's instance for the call p describes (layout, output type, a's flags); false when the
// tile has none.  (Plain if/else and switch, not ?:, between kernel instances -- see the
// explicit-instantiation note above.)
template <int BM, int BN, int WM, int WN, int NST, int KK, bool KKF, bool MIX, int MN, int LEAN>
bool dma_instance(const GemmArgs& a, bool lean_req, bool gen_req, GemmPlan& p) {
  p.BM = BM; p.BN = BN; p.WM = WM; p.WN = WN; p.NST = NST;
  p.block = WM * WN * 64;
  p.group2 = nullptr;
  // fused output sums: bf16 output; the caller's buffer holds 8 partials per 128x128 of output
  // (ops/hip.py psum_slots), which a tile under 128x128 would overrun
  p.psum = a.psum && !p.out_f32 && BM >= 128 && BN >= 128;
  const bool res = a.flags & (kResAdd | kResMask);
  if (p.a_kc && p.b_kc && !p.out_f32) {
    if constexpr (KK == 0) {
      return false;
    } else if constexpr (KK == 1) {
      if (res) return false;
      set_dma<BM, BN, WM, WN, NST, true, true, false>(p);
    } else {
      if (res && KK < 5) return false;
      const int v = epilogue_variant(a, p.psum);
      if (!gen_req && LEAN >= (lean_req ? 1 : 2)) {
        if constexpr (LEAN > 0) {
          p.family = kFamLean;
          p.variant = v;
          p.name = lean_name<BM, BN, WM, WN, NST>();
          LJS_BY_RES(v, LJS_SET_LEAN)
        }
        return true;
      }
      LJS_BY_RES(v, LJS_SET_DMA)
    }
    return true;
  }
  if (res) return false;  // the epilogue operand is in the k-contiguous bf16 instances only
  if (p.a_kc && p.b_kc) {
    if constexpr (KKF) set_dma<BM, BN, WM, WN, NST, true, true, true>(p);
    return KKF;
  }
  if (!p.a_kc && !p.b_kc && p.out_f32) {
    // weight gradients: the plain split-K slab instance (RES 3) when the slabs are f32 and
    // nothing else is asked for
    if constexpr (MN == 2) {
      if ((a.flags & kSlabs) && !(a.flags & (1 | 2 | 8 | 16)) && a.alpha == 1.f) {
        set_dma<BM, BN, WM, WN, NST, false, false, true, 3>(p);
        p.family = kFamSlab;
        p.group2 = gemm_dma_group2_kernel<BM, BN, WM, WN, NST, false, false, true, 3>;
        p.group2_name = dma_name<BM, BN, WM, WN, NST, false, false, true, true>();
        return true;
      }
    }
    if constexpr (MN > 0) set_dma<BM, BN, WM, WN, NST, false, false, true>(p);
    return MN > 0;
  }
  if constexpr (MIX) {
    if (!p.a_kc && !p.b_kc) set_dma<BM, BN, WM, WN, NST, false, false, false>(p);
    else if (p.a_kc && !p.out_f32) set_dma<BM, BN, WM, WN, NST, true, false, false>(p);
    else if (p.a_kc) set_dma<BM, BN, WM, WN, NST, true, false, true>(p);
    else if (!p.out_f32) set_dma<BM, BN, WM, WN, NST, false, true, false>(p);
    else set_dma<BM, BN, WM, WN, NST, false, true, true>(p);
  }
  return MIX;
}
#undef LJS_SET_DMA
#undef LJS_SET_LEAN
#undef LJS_BY_RES

struct TileEntry { int code, demote, unfold; };
inline const TileEntry* find_tile(int code) {
#define LJS_ENTRY(CODE, BM, BN, WM, WN, NST, KK, KKF, MIX, MN, LEAN, DEMOTE, UNFOLD) {CODE, DEMOTE, UNFOLD},
  static const TileEntry table[] = {LJS_GEMM_TILES(LJS_ENTRY)};
#undef LJS_ENTRY
  for (const TileEntry& t : table)
    if (t.code == code) return &t;
  return nullptr;
}
inline bool tile_instance(int code, const GemmArgs& a, bool lean_req, bool gen_req, GemmPlan& p) {
  switch (code) {
#define LJS_CASE(CODE, BM, BN, WM, WN, NST, KK, KKF, MIX, MN, LEAN, DEMOTE, UNFOLD) \
  case CODE: return dma_instance<BM, BN, WM, WN, NST, KK, KKF, MIX, MN, LEAN>(a, lean_req, gen_req, p);
    LJS_GEMM_TILES(LJS_CASE)
#undef LJS_CASE
  }
  return false;
}

// the register-staged tiles (64, 128): the terminal fallbacks, every layout and output type
template <int BM, int BN>
void reg_instance(GemmPlan& p) {
  p.family = kFamReg;
  p.BM = BM; p.BN = BN; p.WM = 2; p.WN = 2; p.NST = 2;
  p.block = 256;
  p.variant = -1;
  p.psum = false;
  p.group2 = nullptr;
#define LJS_CASE(AK, BK_, OF)                                   \
  if (p.a_kc == AK && p.b_kc == BK_ && p.out_f32 == OF) {       \
    p.kernel = gemm_bf16_kernel<BM, BN, AK, BK_, OF>;           \
    p.name = reg_name<BM, BN, AK, BK_, OF>();                   \
  }
  LJS_CASE(1, 1, 0) LJS_CASE(1, 1, 1) LJS_CASE(0, 0, 0) LJS_CASE(0, 0, 1)
  LJS_CASE(1, 0, 0) LJS_CASE(1, 0, 1) LJS_CASE(0, 1, 0) LJS_CASE(0, 1, 1)
#undef LJS_CASE
}

// The LDS-DMA and lean kernels' grid: persistent when the items fill whole rounds of the resident
// slots -- each block then walks `rounds` items with the next item's first K-tiles in flight
// during the current item's epilogue (measured at T = 16384: QKV projection 43.8 -> 39.9 us on
// 128x128 x 2/CU).  Otherwise one block per item, which lets the dispatcher balance a ragged last
// round (measured best at the bench shapes).
inline int dma_grid(const GemmPlan& p, int cus) {
  const int lds_bytes = p.NST * (p.BM + p.BN) * BK * 2;
  const int slots = cus * ((p.WM * p.WN == 4 && lds_bytes <= 80 * 1024) ? 2 : 1);  // resident blocks
  return (p.items > slots && p.items % slots == 0) ? slots : p.items;
}

// a: the call as ljs_gemm_bf16 received it (a.psum: the caller's psum buffer; a.splitk and
// a.kt_per_split are not read).  Preconditions checked here (the Python wrapper checks them too):
// K % 8 == 0; for an m/n-contiguous operand its M (or N) % 8 == 0; leading dimensions that are
// multiples of 8 elements.
GemmPlan gemm_plan(const GemmArgs& a, bool a_kc, bool b_kc, bool out_f32, int splitk, int tile, int cus) {
  GemmPlan p{};
  p.err = hipErrorInvalidValue;
  p.a_kc = a_kc; p.b_kc = b_kc; p.out_f32 = out_f32;
  p.N = a.N; p.batch = a.batch;
  const int M = a.M, N = a.N, K = a.K, flags = a.flags;
  const bool res = flags & (kResAdd | kResMask), slabs = flags & kSlabs;
  if (K % 8 || (!a_kc && M % 8) || (!b_kc && N % 8) || a.lda % 8 || a.ldb % 8) return p;
  if (splitk > 1 && !out_f32) return p;
  // the epilogue operand applies to bf16 outputs (its 16-byte loads need aligned 8-column chunks)
  if (res && (out_f32 || !a.res || (a.ldr % 8) || (a.sR % 8) || (N % 8) || (((uintptr_t)a.res) & 15))) return p;
  // B as a host array of `batch` (<= 4) device pointers: slab mode only
  if ((flags & kBPtrs) && (a.batch < 1 || a.batch > 4 || !slabs)) return p;
  // zeroing C first (split-K accumulates with atomics) needs C to be one dense block
  if ((flags & 16) && a.batch > 1 && a.sC != (long)M * a.ldc) return p;
  const bool gen_req = tile >= 2 * kForceLean;
  if (gen_req) tile -= 2 * kForceLean;
  const bool lean_req = tile >= kForceLean;
  if (lean_req) tile -= kForceLean;
  const int nkt = (K + BK - 1) / BK;
  if (splitk < 1) splitk = 1;
  if (splitk > nkt) splitk = nkt;
  p.kt_per_split = (nkt + splitk - 1) / splitk;
  p.splitk = (nkt + p.kt_per_split - 1) / p.kt_per_split;
  // a split's partial is no output: the kernels would drop a bias (it is added when splitk == 1
  // only) and apply a ReLU to every partial before the atomic add or in every slab
  if ((p.splitk > 1 || slabs) && (flags & 3)) return p;
  // The LDS-DMA kernels need K % 64 == 0, a split that divides the K-tiles (slab mode: the last
  // split may run past K), operands addressable with 32-bit byte offsets and, for a bf16 output,
  // whole aligned 16-byte chunks of C.
  const long k_ext = slabs ? (long)p.splitk * p.kt_per_split * BK : K;  // K-rows the splits address
  const bool dma_ok = K % BK == 0 && (slabs || (K / BK) % p.splitk == 0) &&
                      (a_kc ? (long)M * a.lda : k_ext * a.lda) < (1L << 30) &&
                      (b_kc ? (long)N * a.ldb : k_ext * a.ldb) < (1L << 30);
  const bool dma_store_ok = out_f32 || (N % 8 == 0 && a.ldc % 8 == 0 && (a.sC % 8 == 0 || a.batch == 1) &&
                                        (((uintptr_t)a.C) & 15) == 0);
  // slab mode: f32 slabs of an LDS-DMA tile over m/n-contiguous operands, and the caller's slab
  // count must be the launched split count
  if (slabs && (!out_f32 || a_kc || b_kc || (flags & (8 | 16)) || p.splitk != splitk || !find_tile(tile) || !dma_ok))
    return p;
  // walk the demotion chain to the first tile that has an instance for this call
  while (const TileEntry* t = find_tile(tile)) {
    if (!(dma_ok && dma_store_ok) || !tile_instance(tile, a, lean_req, gen_req, p)) {
      tile = t->demote;
    } else if (t->unfold && a.batch > 1) {
      // weight-major batches side by side in C over contiguous B (the fused Q/K/V projection):
      // one GEMM over N * batch columns (the folded B still addressable by 32-bit offsets)
      if (a.sA == 0 && a.sB == (long)N * a.ldb && a.sC == N && a.ldc == (long)N * a.batch && !a.bias &&
          (long)N * a.batch * a.ldb < (1L << 30)) {
        p.N = N * a.batch;
        p.batch = 1;
        break;
      }
      tile = t->unfold;
    } else {
      break;
    }
  }
  const bool dma = find_tile(tile);
  if (!dma) {
    tile = tile == 64 ? 64 : 128;
    if (tile == 64) reg_instance<64, 64>(p);
    else reg_instance<128, 128>(p);
  }
  const int ntm = (M + p.BM - 1) / p.BM, ntn = (p.N + p.BN - 1) / p.BN;
  if (!dma) {
    p.gx = ntm * ntn;
    p.gy = p.batch * p.splitk;
  } else {
    p.items = ntm * ntn * p.batch * p.splitk;
    p.mfast = ntm < ntn;  // narrow dimension fastest: tiles sharing a panel run together
    p.gx = dma_grid(p, cus);
    p.gy = 1;
    if (p.psum) p.psum_count = p.items * p.WM * p.WN;  // one float per (item, wave)
  }
  p.tile = tile;
  p.err = hipSuccess;
  return p;
}

// ---------------------------------------------------------------------------- launch
inline void gemm_rec(const GemmPlan& p, int req_tile, const char* name, unsigned grid_x, int splitk1 = -1) {
  LjsLaunchRec r = ljs_launch_make(name, dim3(grid_x, p.gy), p.block);
  r.req_tile = req_tile; r.res_tile = p.tile;
  r.splitk = p.splitk; r.splitk1 = splitk1; r.variant = p.variant;
  ljs_launch_push(r);
}

// the call's arguments as its plan launches them
inline void apply_plan(const GemmPlan& p, GemmArgs& a) {
  a.N = p.N;
  a.batch = p.batch;
  a.splitk = p.splitk;
  a.kt_per_split = p.kt_per_split;
  if (!p.psum) a.psum = nullptr;
  if (p.mfast) a.flags |= kMFast;
}

hipError_t launch_plan(const GemmPlan& p, GemmArgs a, int req_tile, hipStream_t s) {
  if (p.family == kFamDma || p.family == kFamSlab) a.trace = g_gemm_trace;
  gemm_rec(p, req_tile, p.name, p.gx);
  void* args[] = {&a};
  (void)hipLaunchKernel((const void*)p.kernel, dim3(p.gx, p.gy), dim3(p.block), args, 0, s);
  return hipGetLastError();
}

// Grouped weight-gradient launches (ljs_gemm_group_begin / _end): while a group is open, plain f32
// slab GEMMs are recorded instead of launched; closing it launches two recorded GEMMs of the same
// kernel instance as ONE grid (gemm_dma_group2_kernel, one block per work item) and anything else
// one by one.  Same kernel body per item: bit-identical to separate launches.
struct GroupRec {
  GemmArgs a;
  GemmPlan p;
  int req_tile;   // for the launch record, as ljs_gemm_bf16 saw it
};
// (per host thread: another thread's GEMMs are never recorded into this thread's open group)
static thread_local bool g_group_on = false;
static thread_local GroupRec g_group[2];
static thread_local int g_group_n = 0;

hipError_t launch_group2(GroupRec* r, hipStream_t s) {
  const GemmPlan& p = r[0].p;
  const unsigned grid = r[0].p.items + r[1].p.items;
  gemm_rec(p, r[0].req_tile, p.group2_name, grid, r[1].p.splitk);
  void* args[] = {&r[0].a, &r[1].a, &r[0].p.items};
  (void)hipLaunchKernel((const void*)p.group2, dim3(grid), dim3(p.block), args, 0, s);
  return hipGetLastError();
}

GemmArgs make_args(const void* A, const void* B, void* C, const void* bias, int M, int N, int K, long lda, long ldb,
                   long ldc, long sA, long sB, long sC, long sBias, int batch, int flags, float alpha, void* psum,
                   const void* res, long ldr, long sR) {
  GemmArgs a{};  // (bptr, trace: null)
  a.A = (const bf16_t*)A; a.B = (const bf16_t*)B; a.C = C; a.bias = bias;
  a.lda = lda; a.ldb = ldb; a.ldc = ldc;
  a.sA = sA; a.sB = sB; a.sC = sC; a.sBias = sBias;
  a.M = M; a.N = N; a.K = K; a.batch = batch;
  a.alpha = alpha; a.flags = flags;
  a.psum = (float*)psum;
  a.res = res; a.ldr = ldr; a.sR = sR;
  return a;
}

}  // namespace

LJS_API void ljs_gemm_group_begin() {
  g_group_on = true;
  g_group_n = 0;
}

// launches what the open group recorded (grouped when it is two GEMMs of one kernel instance)
LJS_API int ljs_gemm_group_end(hipStream_t stream) {
  g_group_on = false;
  const int n = g_group_n;
  g_group_n = 0;
  if (n == 2 && g_group[0].p.kernel == g_group[1].p.kernel) return (int)launch_group2(g_group, stream);
  for (int i = 0; i < n; ++i) {
    const hipError_t e = launch_plan(g_group[i].p, g_group[i].a, g_group[i].req_tile, stream);
    if (e != hipSuccess) return (int)e;
  }
  return 0;
}

// LJS_GEMM_TRACE builds: the LDS-DMA launches that follow write their per-wave timelines to
// `buf` (blocks x waves x kTraceSlots u64, zeroed by the caller); null turns it off.  Returns
// kTraceSlots, or 0 in a library built without the instrumentation.
LJS_API int ljs_gemm_set_trace(void* buf) {
#ifdef LJS_GEMM_TRACE
  g_gemm_trace = (unsigned long long*)buf;
  return kTraceSlots;
#else
  (void)buf;
  return 0;
#endif
}

// Returns 0 on success.  A call the plan rejects returns hipErrorInvalidValue with nothing done:
// C is not zeroed (flags & 16) and nothing is launched or recorded.
LJS_API int ljs_gemm_bf16(const void* A, const void* B, void* C, const void* bias, int M, int N, int K,
                          long lda, long ldb, long ldc, long sA, long sB, long sC, long sBias, int batch,
                          int a_kc, int b_kc, int out_f32, int flags, float alpha, int splitk, int tile,
                          void* psum, int* psum_count, const void* res, long ldr, long sR, hipStream_t stream) {
  GemmArgs a = make_args(A, B, C, bias, M, N, K, lda, ldb, ldc, sA, sB, sC, sBias, batch, flags, alpha, psum, res,
                         ldr, sR);
  const GemmPlan p = gemm_plan(a, a_kc, b_kc, out_f32, splitk, tile, ljs_device_cus());
  if (p.err != hipSuccess) return (int)p.err;
  if (psum_count) *psum_count = p.psum_count;
  if (flags & 16) {  // zero C first (split-K accumulates with atomics)
    const size_t es = out_f32 ? 4 : 2;
    const size_t bytes = ((size_t)(batch - 1) * sC + (size_t)(M - 1) * ldc + N) * es;
    const hipError_t me = hipMemsetAsync(C, 0, bytes, stream);
    if (me != hipSuccess) return (int)me;
  }
  if (flags & kBPtrs) {
    // B is a HOST array of `batch` device pointers, one B operand per batch
    const void* const* bp = (const void* const*)B;
    for (int i = 0; i < 4; ++i) a.bptr[i] = (const bf16_t*)(i < batch ? bp[i] : bp[0]);
    a.B = a.bptr[0];
  }
  apply_plan(p, a);
  if (p.family == kFamSlab && g_group_on && g_group_n < 2) {
    g_group[g_group_n++] = GroupRec{a, p, tile};
    return 0;
  }
  return (int)launch_plan(p, a, tile, stream);
}

// The plan of the same call on a device of `cus` compute units, without a GPU: nothing is
// dereferenced or launched (C and res are read as addresses, for their alignment).  out[0..20]:
// error, resolved tile, family (0 register-staged, 1 LDS-DMA, 2 lean, 3 groupable slab), BM, BN, WM,
// WN, NST, a_kc, b_kc, out_f32, variant, splitk, kt_per_split, launched N, launched batch, grid x,
// grid y, block, psum partials, kMFast; name: the kernel instance.  Returns the error.
LJS_API int ljs_gemm_plan(const void* A, const void* B, void* C, const void* bias, int M, int N, int K, long lda,
                          long ldb, long ldc, long sA, long sB, long sC, long sBias, int batch, int a_kc, int b_kc,
                          int out_f32, int flags, float alpha, int splitk, int tile, void* psum, int* psum_count,
                          const void* res, long ldr, long sR, int cus, int* out, char* name, int name_cap) {
  const GemmPlan p = gemm_plan(make_args(A, B, C, bias, M, N, K, lda, ldb, ldc, sA, sB, sC, sBias, batch, flags, alpha,
                                         psum, res, ldr, sR),
                               a_kc, b_kc, out_f32, splitk, tile, cus);
  if (psum_count) *psum_count = p.psum_count;
  const int v[21] = {(int)p.err, p.tile, p.family, p.BM, p.BN, p.WM, p.WN, p.NST, p.a_kc, p.b_kc, p.out_f32,
                     p.variant, p.splitk, p.kt_per_split, p.N, p.batch, (int)p.gx, (int)p.gy, (int)p.block,
                     p.psum_count, p.mfast};
  for (int i = 0; i < 21; ++i) out[i] = v[i];
  if (name && name_cap > 0) snprintf(name, (size_t)name_cap, "%s", p.err == hipSuccess ? p.name : "");
  return (int)p.err;
}

// ============================================================================ launch record
// The process's launches through gemm.hip / attention.hip so far, and record i of them (0 = the
// first; only the last 32 are kept) as one line of "key=value" text in buf.  Returns the line's
// length, or -1 when record i is no longer (or not yet) there or buf is too small.
LJS_API long ljs_launch_count() {
  std::lock_guard<std::mutex> g(g_ljs_launch_mu);
  return g_ljs_launch_count;
}

LJS_API int ljs_launch_get(long i, char* buf, int cap) {
  std::lock_guard<std::mutex> g(g_ljs_launch_mu);
  if (i < 0 || i >= g_ljs_launch_count || i < g_ljs_launch_count - kLjsLaunchRing || !buf || cap <= 0) return -1;
  const LjsLaunchRec r = g_ljs_launch_ring[i % kLjsLaunchRing];
  const int n = snprintf(buf, (size_t)cap,
                         "name=%s grid=%u,%u,%u block=%u requested_tile=%d resolved_tile=%d splitk=%d splitk1=%d "
                         "variant=%d acc_mode=%d",
                         r.name, r.gx, r.gy, r.gz, r.block, r.req_tile, r.res_tile, r.splitk, r.splitk1, r.variant,
                         r.acc_mode);
  return n < cap ? n : -1;
}

// ============================================================================ f32 GEMM
// Exact-f32 GEMM on the f32-input MFMA (v_mfma_f32_16x16x4_f32: a k-ordered fmaf chain, no
// reduced-precision path).  Arbitrary element strides, so any transpose is free; operands are
// read straight from global (this serves the small f32 matmuls of cases 1-4 and generic
// f32 dot_general; large GEMMs run in bf16 above).  One wave per 16x16 output tile, 2x2 waves.
namespace {
struct GemmF32Args {
  const float* A; const float* B; float* C;
  long a_rs, a_cs, b_rs, b_cs, c_rs;
  long sA, sB, sC;
  int M, N, K;
};

__global__ __launch_bounds__(256) void gemm_f32_kernel(GemmF32Args p) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int m0 = blockIdx.x * 32 + (wave >> 1) * 16, n0 = blockIdx.y * 32 + (wave & 1) * 16;
  const int b = blockIdx.z;
  const float* A = p.A + b * p.sA;
  const float* B = p.B + b * p.sB;
  const int am = m0 + (lane & 15), bn = n0 + (lane & 15), kk = lane >> 4;
  f32x4 acc = {0.f, 0.f, 0.f, 0.f};
  for (int k0 = 0; k0 < p.K; k0 += 4) {
    const int k = k0 + kk;
    float a = (am < p.M && k < p.K) ? A[am * p.a_rs + k * p.a_cs] : 0.f;
    float bb = (bn < p.N && k < p.K) ? B[k * p.b_rs + bn * p.b_cs] : 0.f;
    acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a, bb, acc, 0, 0, 0);
  }
  const int col = n0 + (lane & 15);
  if (col >= p.N) return;
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int row = m0 + (lane >> 4) * 4 + r;
    if (row < p.M) p.C[b * p.sC + row * p.c_rs + col] = acc[r];
  }
}
}  // namespace

LJS_API int ljs_gemm_f32(const void* A, const void* B, void* C, int M, int N, int K, long a_rs, long a_cs, long b_rs,
                         long b_cs, long c_rs, long sA, long sB, long sC, int batch, hipStream_t stream) {
  GemmF32Args p;
  p.A = (const float*)A; p.B = (const float*)B; p.C = (float*)C;
  p.a_rs = a_rs; p.a_cs = a_cs; p.b_rs = b_rs; p.b_cs = b_cs; p.c_rs = c_rs;
  p.sA = sA; p.sB = sB; p.sC = sC;
  p.M = M; p.N = N; p.K = K;
  dim3 grid((M + 31) / 32, (N + 31) / 32, batch);
  ljs_launch_rec("gemm_f32", grid, 256);
  hipLaunchKernelGGL(gemm_f32_kernel, grid, dim3(256), 0, stream, p);
  return (int)hipGetLastError();
}
