// What the two weight-streaming skinny GEMMs share (skinny.hip: bf16 weights; skinny_mx.hip: MX-fp8 weights):
// the bounds of the layout, the epilogue flags, the epilogue itself, the launch names and the tests' forced
// wave count.
#pragma once
#include "common.h"
#include <string>

constexpr int kSkMaxM = 16;
constexpr int kSkCols = 16;              // output columns per block
constexpr int kSkMaxWaves = 16;
constexpr int kSkWavesPerCu = 8;         // the plans' target

constexpr int kSkBias = 1, kSkBiasF32 = 2, kSkRelu = 4, kSkRes = 8, kSkResF32 = 16, kSkOutF32 = 32;

// > 0: a wave count forced by tests (ljs_skinny_set_waves, skinny.hip), for both kernels
int ljs_skinny_forced_waves();

inline bool sk_waves_ok(int w) { return w == 1 || w == 2 || w == 4 || w == 8 || w == 16; }

// what a launch writes and adds: y and res [M][N] with their leading dimensions, bias [N]
struct SkinnyEpi {
  void* y;
  const void *bias, *res;
  long ldc, ldr;
  int M, N, flags;
};

// The epilogue of one lane: its 4 accumulators are row m, columns n .. n + 3 of the product.  In this order:
// + bias in f32 (bias f32 or bf16), ReLU, the rounding to bf16 (or the f32 store), then the residual as the
// tile kernels add it (gemm.hip apply_res8): bf16(bf16(y) + bf16(res)), bf16 output only.
__device__ __forceinline__ void skinny_epilogue(const SkinnyEpi& a, const f32x4& acc, const int m, const int n) {
  if (m >= a.M || n >= a.N) return;                    // (N % 4 == 0: a lane's 4 columns are whole)
  float v[4] = {acc[0], acc[1], acc[2], acc[3]};
  if (a.flags & kSkBias) {
    float b[4];
    if (a.flags & kSkBiasF32) {
#pragma unroll
      for (int e = 0; e < 4; ++e) b[e] = reinterpret_cast<const float*>(a.bias)[n + e];
    } else {
#pragma unroll
      for (int e = 0; e < 4; ++e) b[e] = bf2f(reinterpret_cast<const bf16_t*>(a.bias)[n + e]);
    }
#pragma unroll
    for (int e = 0; e < 4; ++e) v[e] += b[e];
  }
  if (a.flags & kSkRelu) {
#pragma unroll
    for (int e = 0; e < 4; ++e) v[e] = fmaxf(v[e], 0.f);
  }
  if (a.flags & kSkOutF32) {
    *reinterpret_cast<f32x4*>(reinterpret_cast<float*>(a.y) + (long)m * a.ldc + n) = f32x4{v[0], v[1], v[2], v[3]};
    return;
  }
  if (a.flags & kSkRes) {
    float r[4];
    if (a.flags & kSkResF32) {
      const f32x4 rf = *reinterpret_cast<const f32x4*>(reinterpret_cast<const float*>(a.res) + (long)m * a.ldr + n);
#pragma unroll
      for (int e = 0; e < 4; ++e) r[e] = rf[e];
    } else {
      const u32x2 rb = *reinterpret_cast<const u32x2*>(reinterpret_cast<const bf16_t*>(a.res) + (long)m * a.ldr + n);
#pragma unroll
      for (int e = 0; e < 2; ++e) {
        r[2 * e] = __uint_as_float(rb[e] << 16);
        r[2 * e + 1] = __uint_as_float(rb[e] & 0xffff0000u);
      }
    }
#pragma unroll
    for (int e = 0; e < 4; ++e) v[e] = bf2f(f2bf(v[e])) + bf2f(f2bf(r[e]));
  }
  *reinterpret_cast<u32x2*>(reinterpret_cast<bf16_t*>(a.y) + (long)m * a.ldc + n) =
      u32x2{pack_bf16x2(v[0], v[1]), pack_bf16x2(v[2], v[3])};
}

// the partial accumulators of a block's W waves, added by wave 0 IN WAVE ORDER through LDS (16 bytes per
// lane, conflict-free); false for the waves that are done.  A one-wave block touches no LDS.
__device__ __forceinline__ bool skinny_reduce(f32x4* part, f32x4& acc, const int wave, const int lane, const int W) {
  if (W == 1) return true;
  part[wave * 64 + lane] = acc;
  __syncthreads();
  if (wave != 0) return false;
  acc = part[lane];
  for (int w = 1; w < W; ++w) acc += part[w * 64 + lane];
  return true;
}

inline int sk_epi_flags(const void* bias, const void* res, int out_f32, int bias_f32, int res_f32, int relu) {
  return (bias ? kSkBias : 0) | (bias && bias_f32 ? kSkBiasF32 : 0) | (relu ? kSkRelu : 0) | (res ? kSkRes : 0) |
         (res && res_f32 ? kSkResF32 : 0) | (out_f32 ? kSkOutF32 : 0);
}

// the launchers' checks of y, bias and res (what skinny_epilogue reads and writes)
inline bool sk_epi_ok(const void* y, const void* bias, const void* res, int N, long ldc, long res_ld, int out_f32,
                      int bias_f32, int res_f32) {
  if (!y || ldc < N || ldc % 4 || (((uintptr_t)y) & (out_f32 ? 15u : 7u))) return false;
  if (bias && (((uintptr_t)bias) & (bias_f32 ? 3u : 1u))) return false;
  if (res && (out_f32 || res_ld < N || res_ld % 4 || (((uintptr_t)res) & (res_f32 ? 15u : 7u)))) return false;
  return true;
}

// "<prefix><W,out[,bias][,relu][,res]>": one string per (wave count, flag set), made once per prefix
inline std::string* sk_make_names(const char* prefix) {
  auto* t = new std::string[5 * 16];
  const int ws[5] = {1, 2, 4, 8, 16};
  for (int i = 0; i < 5; ++i)
    for (int f = 0; f < 16; ++f)
      t[i * 16 + f] = std::string(prefix) + "<" + std::to_string(ws[i]) + (f & 1 ? ",f32" : ",bf16") +
                      (f & 2 ? ",bias" : "") + (f & 4 ? ",relu" : "") + (f & 8 ? ",res" : "") + ">";
  return t;
}
inline const char* sk_name(const std::string* table, int waves, int flags) {
  const int i = waves == 1 ? 0 : waves == 2 ? 1 : waves == 4 ? 2 : waves == 8 ? 3 : 4;
  const int f = (flags & kSkOutF32 ? 1 : 0) | (flags & kSkBias ? 2 : 0) | (flags & kSkRelu ? 4 : 0) |
                (flags & kSkRes ? 8 : 0);
  return table[i * 16 + f].c_str();
}
