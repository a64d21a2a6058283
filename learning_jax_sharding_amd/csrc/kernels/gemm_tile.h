// What the tile GEMMs share (gemm.hip: bf16 operands; gemm_w8.hip: bf16 x, MX-fp8 weights): the call's
// arguments, the epilogue operand, the swizzled LDS images of one 64-deep K-tile, their LDS-DMA pieces and
// their MFMA fragment reads.  Every function is forced inline: each file compiles to the code it had with
// these lines in it.
#pragma once
#include "common.h"

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

constexpr int kResAdd = 64, kResMask = 128, kResF32 = 256;

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

// XOR applied to the 16-byte chunk index of k-row `krow` of an m/n-contiguous image (R rows)
template <int R>
__device__ __forceinline__ int swz_mn16(int krow) {
  // (rows of 128 or 256 bf16 start on the same bank; rows of 64 alternate halves)
  if constexpr (R >= 128) return ((krow & 3) | (((krow >> 3) & 1) << 2)) << 1;
  else return ((((krow >> 1) & 1)) | (((krow >> 3) & 1) << 1)) << 1;
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

constexpr int kSC1 = 16;  // buffer-instruction cache policy bit: sc1 (gfx940-family CPol::SC1)

}  // namespace
