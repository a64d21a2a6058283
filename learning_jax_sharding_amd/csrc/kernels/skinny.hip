// Weight-streaming skinny GEMM for the decode projections: y[m][n] = epi(sum_k x[m][k] Wt[n][k]) for
// 1 <= M <= 16 rows of activations, K % 32 == 0, N % 8 == 0.  Forward only.
//
// Operands.  x is bf16 [M][K] with row stride lda; Wt is the dense layer's bf16 transposed weight
// shadow [N][K] (k-contiguous, row stride ldb; a fused projection's stacked shadows are one
// [nw * N][K] operand); y is bf16 or f32 with row stride ldc >= N (a column block of a wider buffer).
// Rows of x and Wt are 16-byte aligned, offsets are 64-bit.
//
// Every decode GEMM reads its whole weight once for at most 16 rows, so this is not a tile pipeline:
// the weight goes from memory straight to VGPRs (no LDS image, no barrier per K-tile) and the
// v_mfma_f32_16x16x32_bf16 runs with the WEIGHT as its A operand and x as its B operand:
//     lane l holds 16 bytes of weight row n0 + (l & 15) at k-chunk 4 s + (l >> 4) of K-step s,
//     and the same 16 bytes of x row l & 15 (zeros BY SELECT for rows >= M: they are never loaded,
//     so whatever lies behind x cannot reach a sum as 0 * NaN);
//     D then has col = m = l & 15 and the 4 consecutive n = n0 + 4 (l >> 4) + 0..3 per lane,
// so a lane stores 8 bytes of bf16 (16 of f32) into output row m.  The four 16-lane groups of one load
// cover 64 contiguous bytes of each of 16 weight rows, and two K-steps one whole 128-byte line of each.
//
// One block per group of 16 output columns.  Its W waves split K in units of step PAIRS (one 128-byte
// line per weight row), evenly (wave w takes pairs [w P / W, (w + 1) P / W), P = ceil(K / 64)), so a
// wave's back-to-back loads cover whole lines and no line is fetched by two waves.  A wave issues the
// loads of up to kSkUnroll steps (weight and x) before its first MFMA; there is nothing else to wait
// behind.  The partial accumulators go through LDS (16 bytes per lane, conflict-free; dynamic, 1 KiB per
// wave, none for a one-wave block) and wave 0 adds
// them IN WAVE ORDER, so the bits do not depend on timing; a wave whose slice is empty (K = 32 with
// W > 1, or a forced wave count above the pair count) contributes zeros.  No atomics, no workspace, no
// memset, no ticket: nothing to re-arm for a graph replay.
//
// The last column group of an N that is no multiple of 16 clamps its weight row to N - 1 for the loads
// and does not store the clamped columns.  No load touches memory outside rows [0, N) x columns [0, K)
// of Wt or rows [0, M) of x.
//
// Epilogue, in this order: + bias in f32 (bias f32 or bf16), ReLU, the rounding to bf16 (or the f32
// store), then the residual as the tile kernels add it (gemm.hip apply_res8): bf16(bf16(y) +
// bf16(res)), res f32 or bf16 with its own leading dimension, bf16 output only.  Alpha is 1; there is
// no accumulate, no split-K slab, no mask mode and no fused output sum.
//
// The plan (skinny_plan: of N, K and the CU count, nothing else; M does not enter it).  blocks =
// ceil(N / 16) is fixed by the layout; the wave count is what decides how many bytes are in flight:
//     W = min(16, pow2floor(P), pow2ceil(ceil(kSkWavesPerCu * cus / blocks)))
// - never more waves than step pairs (hence never more than K-steps): a wave without a line to fetch
//   only adds a partial to the reduction;
// - short-N projections (the 16 .. 40 blocks of a 256 / 512 / 640-column projection on 256 CUs) get
//   the most waves their K allows, so that all of the weight is requested in the first round of loads
//   instead of a few waves walking K one latency at a time;
// - from kSkWavesPerCu = 8 waves per CU on (two per SIMD: 64 KiB of weight in flight per CU at 8 steps
//   each, above the ~10 MB the chip needs in flight to stream at its rate) more waves only shorten
//   each wave's run and lengthen the reduction, so the vocabulary head's 2048 blocks run one wave each.
// The rule rests on this latency / bytes-in-flight argument; the measured figures are in
// profiles/PERF_NOTES.md ("Skinny GEMM").  It is monotone: W does not grow with N, does not shrink
// with K or with the CU count.
#include "common.h"
#include <string>

namespace {

constexpr int kSkMaxM = 16;
constexpr int kSkCols = 16;              // output columns per block
constexpr int kSkMaxWaves = 16;
constexpr int kSkUnroll = 8;             // K-steps whose loads a wave has in flight together
constexpr int kSkWavesPerCu = 8;         // the plan's target

constexpr int kSkBias = 1, kSkBiasF32 = 2, kSkRelu = 4, kSkRes = 8, kSkResF32 = 16, kSkOutF32 = 32;

int g_sk_waves = 0;                      // > 0: a wave count forced by tests

struct SkinnyArgs {
  const bf16_t *x, *wt;
  void* y;
  const void *bias, *res;
  long lda, ldb, ldc, ldr;
  int M, N, K, flags;
};

// the loads of CNT K-steps (weight and x) first, then their MFMAs; FULL: CNT == kSkUnroll (no tests)
template <bool FULL>
__device__ __forceinline__ void skinny_steps(const bf16_t* wp, const bf16_t* xp, const bool xok, const int cnt,
                                             f32x4& acc) {
  u32x4 wv[kSkUnroll], xv[kSkUnroll];
#pragma unroll
  for (int u = 0; u < kSkUnroll; ++u) {
    if (FULL || u < cnt) wv[u] = *reinterpret_cast<const u32x4*>(wp + u * 32);
  }
#pragma unroll
  for (int u = 0; u < kSkUnroll; ++u) {
    xv[u] = u32x4{0u, 0u, 0u, 0u};
    if ((FULL || u < cnt) && xok) xv[u] = *reinterpret_cast<const u32x4*>(xp + u * 32);
  }
#pragma unroll
  for (int u = 0; u < kSkUnroll; ++u) {
    if (FULL || u < cnt)
      acc = mfma16x16x32(__builtin_bit_cast(bf16x8, wv[u]), __builtin_bit_cast(bf16x8, xv[u]), acc);
  }
}

__global__ __launch_bounds__(kSkMaxWaves * 64)
void skinny_kernel(const SkinnyArgs a) {
  extern __shared__ f32x4 part[];                      // [W][64], dynamic: none for a one-wave block
  const int lane = threadIdx.x & 63, g = lane >> 4, r16 = lane & 15;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int W = (int)(blockDim.x >> 6);
  const int n0 = blockIdx.x * kSkCols;

  const int steps = a.K >> 5, pairs = (steps + 1) >> 1;
  const int lgw = __builtin_ctz((unsigned)W);          // W is a power of two (the launcher)
  const int p0 = (wave * pairs) >> lgw, p1 = ((wave + 1) * pairs) >> lgw;
  const int s0 = 2 * p0, s1 = 2 * p1 < steps ? 2 * p1 : steps;

  int nrow = n0 + r16;
  nrow = nrow < a.N ? nrow : a.N - 1;                 // the tail group: clamped for the loads, not stored
  const bool xok = r16 < a.M;
  const bf16_t* wp = a.wt + (long)nrow * a.ldb + (long)(s0 * 4 + g) * 8;
  const bf16_t* xp = a.x + (long)(xok ? r16 : 0) * a.lda + (long)(s0 * 4 + g) * 8;

  f32x4 acc = {0.f, 0.f, 0.f, 0.f};
  for (int s = s0; s < s1; s += kSkUnroll) {
    const int cnt = s1 - s;                            // (wave-uniform)
    if (cnt >= kSkUnroll) skinny_steps<true>(wp, xp, xok, kSkUnroll, acc);
    else skinny_steps<false>(wp, xp, xok, cnt, acc);
    wp += kSkUnroll * 32;
    xp += kSkUnroll * 32;
  }

  if (W > 1) {
    part[wave * 64 + lane] = acc;
    __syncthreads();
    if (wave != 0) return;
    acc = part[lane];
    for (int w = 1; w < W; ++w) acc += part[w * 64 + lane];  // in wave order
  }

  const int n = n0 + 4 * g, m = r16;
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

inline bool sk_waves_ok(int w) { return w == 1 || w == 2 || w == 4 || w == 8 || w == 16; }

inline bool sk_shape_ok(int M, int N, int K) {
  return M >= 1 && M <= kSkMaxM && N >= 8 && N % 8 == 0 && K >= 32 && K % 32 == 0;
}

// the pure plan: (waves per block, blocks) of a shape on `cus` compute units (the head of the file)
inline void skinny_plan(int N, int K, int cus, int* waves, int* blocks) {
  const long nb = ((long)N + kSkCols - 1) / kSkCols;
  const int pairs = (K / 32 + 1) / 2;
  const long want = ((long)kSkWavesPerCu * cus + nb - 1) / nb;
  int w = 1;
  while (w < kSkMaxWaves && w < want) w *= 2;          // pow2ceil(want), at most 16
  while (w > pairs) w /= 2;                            // at most pow2floor(pairs)
  *waves = w < 1 ? 1 : w;
  *blocks = (int)nb;
}

// "skinny<W,out[,bias][,relu][,res]>": one string per (wave count, flag set), made once
const char* skinny_name(int waves, int flags) {
  static const std::string* table = [] {
    auto* t = new std::string[5 * 16];
    const int ws[5] = {1, 2, 4, 8, 16};
    for (int i = 0; i < 5; ++i)
      for (int f = 0; f < 16; ++f)
        t[i * 16 + f] = "skinny<" + std::to_string(ws[i]) + (f & 1 ? ",f32" : ",bf16") + (f & 2 ? ",bias" : "") +
                        (f & 4 ? ",relu" : "") + (f & 8 ? ",res" : "") + ">";
    return t;
  }();
  const int i = waves == 1 ? 0 : waves == 2 ? 1 : waves == 4 ? 2 : waves == 8 ? 3 : 4;
  const int f = (flags & kSkOutF32 ? 1 : 0) | (flags & kSkBias ? 2 : 0) | (flags & kSkRelu ? 4 : 0) |
                (flags & kSkRes ? 8 : 0);
  return table[i * 16 + f].c_str();
}

}  // namespace

// out[0] = waves per block, out[1] = blocks of (M, N, K) on a device of `cus` compute units: pure.
// hipErrorInvalidValue for a shape outside 1 <= M <= 16, K % 32 == 0, N % 8 == 0.
LJS_API int ljs_skinny_plan(int M, int N, int K, int cus, int* out) {
  if (!sk_shape_ok(M, N, K) || cus < 1 || !out) return (int)hipErrorInvalidValue;
  skinny_plan(N, K, cus, out, out + 1);
  return 0;
}

// tests: force `n` waves per block (1, 2, 4, 8 or 16; anything else is refused and changes nothing);
// n <= 0 restores the plan
LJS_API int ljs_skinny_set_waves(int n) {
  if (n > 0 && !sk_waves_ok(n)) return (int)hipErrorInvalidValue;
  g_sk_waves = n > 0 ? n : 0;
  return 0;
}

// y [M][N] (ldc) = epi(x [M][K] (lda) . Wt [N][K] (ldb)^T): the head of the file.  bias: null, or N values
// (bias_f32: f32, else bf16); res: null, or [M][N] (res_ld) f32 (res_f32) or bf16, bf16 output only.
// Returns hipErrorInvalidValue, and launches and records nothing, for a shape outside the bounds, a
// null x / Wt / y, leading dimensions below the row length, rows of x or Wt that are not 16-byte
// aligned, y or res not aligned to a lane's 4 values (8 bytes of bf16, 16 of f32), a misaligned bias,
// or a residual with an f32 output.
LJS_API int ljs_skinny_bf16(const void* x, const void* wt, void* y, const void* bias, const void* res, int M, int N,
                            int K, long lda, long ldb, long ldc, long res_ld, int out_f32, int bias_f32, int res_f32,
                            int relu, hipStream_t st) {
  if (!sk_shape_ok(M, N, K) || !x || !wt || !y) return (int)hipErrorInvalidValue;
  if (lda < K || ldb < K || ldc < N || lda % 8 || ldb % 8 || ldc % 4 || (((uintptr_t)x) & 15u) ||
      (((uintptr_t)wt) & 15u) || (((uintptr_t)y) & (out_f32 ? 15u : 7u)))
    return (int)hipErrorInvalidValue;
  if (bias && (((uintptr_t)bias) & (bias_f32 ? 3u : 1u))) return (int)hipErrorInvalidValue;
  if (res && (out_f32 || res_ld < N || res_ld % 4 || (((uintptr_t)res) & (res_f32 ? 15u : 7u))))
    return (int)hipErrorInvalidValue;
  SkinnyArgs a{};
  a.x = (const bf16_t*)x;
  a.wt = (const bf16_t*)wt;
  a.y = y;
  a.bias = bias;
  a.res = res;
  a.lda = lda; a.ldb = ldb; a.ldc = ldc; a.ldr = res_ld;
  a.M = M; a.N = N; a.K = K;
  a.flags = (bias ? kSkBias : 0) | (bias && bias_f32 ? kSkBiasF32 : 0) | (relu ? kSkRelu : 0) | (res ? kSkRes : 0) |
            (res && res_f32 ? kSkResF32 : 0) | (out_f32 ? kSkOutF32 : 0);
  int waves, blocks;
  skinny_plan(N, K, ljs_device_cus(), &waves, &blocks);
  if (g_sk_waves > 0) waves = g_sk_waves;
  const dim3 grid((unsigned)blocks);
  const size_t lds = waves > 1 ? (size_t)waves * 64 * sizeof(f32x4) : 0;
  hipLaunchKernelGGL(skinny_kernel, grid, dim3((unsigned)waves * 64), lds, st, a);
  const int rc = (int)hipGetLastError();
  if (rc == 0) ljs_launch_rec(skinny_name(waves, a.flags), grid, (unsigned)waves * 64);   // a failed launch leaves no record
  return rc;
}
