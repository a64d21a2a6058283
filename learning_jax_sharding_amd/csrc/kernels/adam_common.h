// The fused Adam's tensor table and gradient-source loads, shared by the multi-tensor Adam
// (elementwise.hip) and the gradient sum of squares that reads the same table (clip.hip).
#pragma once
#include "rowwise.h"

// 4 consecutive slab elements as f32 from f32 or bf16 slabs (bf16 slabs: the weight-gradient
// GEMM's split-K partials rounded once each, summed here in f32)
template <typename ST>
__device__ __forceinline__ f32x4 ld_slab4(const ST* __restrict__ p, long e) {
  // global (not flat) loads: they retire in order, so a loop can wait for an older group with a
  // counted vmcnt while a younger one is in flight (a flat load forces vmcnt(0) + lgkmcnt(0))
  if constexpr (sizeof(ST) == 4) {
    return *(const __attribute__((address_space(1))) f32x4*)(reinterpret_cast<const float*>(p) + e);
  } else {
    const u32x2 r = *(const __attribute__((address_space(1))) u32x2*)(reinterpret_cast<const bf16_t*>(p) + e);
    return unpack_bf16x4(r);
  }
}

// Multi-tensor Adam over 64x64 tiles of up to 32 parameters per launch (pointers passed by value
// in the kernel arguments, so the launch is HIP-graph capturable).  Besides p/m/v (in place) it
// refreshes the parameter's bf16 "shadows" used by the next step's MFMA GEMMs: the plain [R][C]
// copy and the transposed [C][R] copy (staged through LDS so both writes are coalesced).  This
// removes every per-step f32->bf16 weight cast kernel from the training step.
struct AdamTensor {
  long p, g, m, v, st, sn, R, C, g_bf16, tiles_c, vec;  // vec: 4-wide path allowed (C % 4, alignment)
  // MX-fp8 shadows of the new weight (0 = none; R, C % 64 == 0, 64-row tiles, vec path):
  // qn[R][C] + sn8[R][C/32] (blocks along rows, quant_mx_rows' layout: a dX GEMM's B operand)
  // and qt[C][R] + st8[C][R/32] (blocks along columns, transposed: a forward GEMM's B operand)
  long qn, sn8, qt, st8;
  // gradient source: gS = 0 a plain [R][C] tensor (row stride g_ld = C); gS > 0 the gS f32
  // split-K slabs of a weight-gradient GEMM, g_ss floats apart, row stride g_ld (the gradient is
  // their sum, added in slab_reduce's order: bit-identical, and no combine launch); gS = -1 a
  // constant gradient whose f32 bits are g_ld (the bias gradient of a loss-sum cotangent)
  long gS, g_ld, g_ss;
  long trows;   // tile height: the launch's kAdamRows, or 16 / 32 (4-wide path, C % 64 == 0)
};
constexpr int kAdamMax = 32;

// table row (16 int64, ops/hip.py adam_multi) -> the tensor's shape and gradient source; false
// when the source's strides are invalid
inline bool adam_grad_from_row(const long* r, AdamTensor& t) {
  t.g = r[1]; t.R = r[6]; t.C = r[7]; t.g_bf16 = r[8];
  t.gS = r[9]; t.g_ld = r[14]; t.g_ss = r[15];
  if (t.gS == 0) t.g_ld = t.C;
  if (t.gS > 0 && (t.g_ld < t.C || t.g_ss < 1)) return false;   // (g_bf16: bf16 slabs)
  t.tiles_c = (t.C + 63) / 64;
  return true;
}
// the gradient source's share of the 4-wide path's conditions
inline bool adam_grad_vec_ok(const AdamTensor& t) {
  auto al = [](long ptr, long a) { return ptr % a == 0; };
  return t.C % 4 == 0 &&
         (t.gS < 0 || (al(t.g, t.g_bf16 ? 8 : 16) && t.g_ld % 4 == 0 && (t.gS == 0 || t.g_ss % 4 == 0)));
}

// the slab sum of slab_reduce_kernel, in its order (bit-identical results)
template <typename ST>
__device__ __forceinline__ float slab_sum1(const ST* __restrict__ g, long gS, long ss, long i) {
  auto ld = [&](long j) {
    if constexpr (sizeof(ST) == 4) return reinterpret_cast<const float*>(g)[j];
    else return bf2f(reinterpret_cast<const bf16_t*>(g)[j]);
  };
  float acc = ld(i);
  long s = 1;
  for (; s + 3 < gS; s += 4) acc += (ld(s * ss + i) + ld((s + 1) * ss + i)) + (ld((s + 2) * ss + i) + ld((s + 3) * ss + i));
  for (; s < gS; ++s) acc += ld(s * ss + i);
  return acc;
}
// the same sum over 4 consecutive elements (slab_reduce_kernel's loop itself)
template <typename ST>
__device__ __forceinline__ f32x4 slab_sum4(const ST* __restrict__ g, long gS, long ss, long i) {
  f32x4 acc = ld_slab4(g, i);
  long s = 1;
  for (; s + 3 < gS; s += 4) {
    const f32x4 v0 = ld_slab4(g, s * ss + i), v1 = ld_slab4(g, (s + 1) * ss + i);
    const f32x4 v2 = ld_slab4(g, (s + 2) * ss + i), v3 = ld_slab4(g, (s + 3) * ss + i);
    acc += (v0 + v1) + (v2 + v3);
  }
  for (; s < gS; ++s) acc += ld_slab4(g, s * ss + i);
  return acc;
}

// The record the optimizer's step_hyper launch (clip.hip) leaves for the dynamic Adam instance:
// the clipping scale of the gradients, the step's learning rate, and the gradients' global norm
struct StepHyper {
  float grad_scale, lr, norm, pad;
};
