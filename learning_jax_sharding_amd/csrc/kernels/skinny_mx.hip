// LJS_HIPCC_FLAGS: -Xclang -target-feature -Xclang -packed-fp32-ops
// Weight-streaming skinny GEMM on MX-fp8 weights (W8A16): y[m][n] = epi(sum_k x[m][k] W_hat[n][k]) for
// 1 <= M <= 16 rows of bf16 activations, K % 128 == 0, N % 8 == 0, with
//     W_hat[n][k] = e4m3(q[n][k]) * 2^(s[n][k / 32] - 127),
// the "QT" shadow of a dense layer's weight (ops/shadow.get_mx: e4m3 codes [N][K], row stride ldq, and e8m0
// scale bytes [N][K / 32], row stride lds, blocks along K; a fused projection's stacked shadows are one
// [nw * N][K] operand).  x is never quantised.  W_hat is an exact bf16 value (4 significant bits times a power
// of two), so the product is the bf16 kernel's (skinny.hip) on the dequantised weight, bit for bit, for half
// the weight bytes plus one scale byte per 32.  Forward only.  Code rows are 16-byte aligned, scale rows 4-byte
// aligned, x rows 16-byte aligned, offsets are 64-bit.
//
// As in skinny.hip there is no LDS image and no barrier per K-tile: the codes go from memory to VGPRs, are
// turned into packed bf16 there by the gfx950 scaled conversion v_cvt_scalef32_pk_bf16_fp8 (no f32 detour:
// one conversion per two codes, the block scale as its f32 operand) and feed v_mfma_f32_16x16x32_bf16 as
// its A operand, x as its B operand.
//
// The unit of K is one LINE: 128 codes = one 128-byte line of a weight row = 4 MX blocks = 4 MFMAs.
//     lane l = (g = l >> 4, r = l & 15) holds codes [32 g, 32 g + 32) of the line of row n0 + r: two 16-byte
//     loads, the four 16-lane groups of a wave covering the whole line of each of 16 rows, and all of a
//     lane's codes inside ONE MX block (block g of the line), so one scale feeds all 16 of its conversions;
//     MFMA j of the line takes the lane's codes [8 j, 8 j + 8) as A and x[r][128 line + 32 g + 8 j ..+8) as B:
//     the MFMA sums over k, so the bijection (MFMA j, lane group g, element i) -> k = 32 g + 8 j + i, shared
//     by both operands, is as good as the natural one.  The lane's x is 64 contiguous bytes per line (four
//     16-byte loads), zeros BY SELECT for rows >= M: they are never loaded.
// D has col = m = l & 15 and the 4 consecutive n = n0 + 4 (l >> 4) + 0..3 per lane, as in skinny.hip, and the
// epilogue is that kernel's (skinny_common.h: one function, both kernels).
//
// Scales: one dword per (row, line) -- the line's four scale bytes, 4-byte aligned because K % 128 == 0 and
// the rows are -- with byte g selected in-lane (a shift by 8 g), loaded with the line's codes.  Loading a
// wave's whole scale slice up front was the alternative; it needs a register count that depends on K / W
// (or a second loop), and the dword rides in the same round of loads as the 32 bytes of codes it scales, from
// a line the four groups of the wave share, so there is no dependent load in front of a conversion.
//
// In flight: a wave issues the loads of up to kMxUnroll = 4 lines (codes, scales, x) before its first
// conversion: 128 bytes of codes per lane, 8 KiB per wave, the weight bytes skinny.hip's kSkUnroll = 8 steps
// keep in flight -- the plan below puts the same 8 waves on a CU, so the same 64 KiB of weight per CU (above
// the ~10 MB the chip needs in flight to stream at its rate) now cover twice the K.  More lines would not
// fit: 4 lines are 32 VGPRs of codes, 4 of scales and 64 of x, and a 16-wave block leaves a lane 128.
//
// One block per 16 output columns.  Its W waves split K evenly in lines (wave w takes lines [w P / W,
// (w + 1) P / W), P = K / 128); partials go through LDS and wave 0 adds them IN WAVE ORDER (skinny_reduce);
// a wave with an empty slice (P < W under a forced wave count) contributes zeros.  No atomics, no
// workspace, nothing to re-arm for a graph replay.  The last column group of an N that is no multiple of
// 16 clamps its row to N - 1 for the code and scale loads and stores nothing there.  No load leaves
// [0, N) x [0, K) of the codes, [0, N) x [0, K / 32) of the scales or the first M rows x [0, K) of x.
//
// The plan (skinny_mx_plan) is skinny.hip's with lines in place of step pairs:
//     W = min(16, pow2floor(K / 128), pow2ceil(ceil(8 cus / blocks))),  blocks = ceil(N / 16);
// pure, M does not enter it, monotone the same way (W does not grow with N, does not shrink with K or the CU
// count).  A wave count forced by ljs_skinny_set_waves holds here too.  Measured figures:
// profiles/PERF_NOTES.md ("MX-fp8 skinny GEMM").
#include "skinny_common.h"

namespace {

constexpr int kMxLine = 128;             // codes (bytes) of a weight row per line
constexpr int kMxUnroll = 4;             // lines whose loads a wave has in flight together

struct SkinnyMxArgs {
  const bf16_t* x;
  const unsigned char *q, *s;
  SkinnyEpi e;
  long lda, ldq, lds;
  int K;
};

// two e4m3 codes (the low or the high half of w) times the f32 scale -> packed bf16, exact
__device__ __forceinline__ unsigned mx_cvt2(unsigned w, float scale, bool hi) {
  return hi ? __builtin_bit_cast(unsigned, __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(w, scale, true))
            : __builtin_bit_cast(unsigned, __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(w, scale, false));
}

// the loads of CNT lines (codes, scales, x) first, then their conversions and MFMAs; FULL: CNT == kMxUnroll
template <bool FULL>
__device__ __forceinline__ void skinny_mx_lines(const unsigned char* qp, const unsigned char* sp, const bf16_t* xp,
                                                const bool xok, const int g, const int cnt, f32x4& acc) {
  u32x4 qv[kMxUnroll][2], xv[kMxUnroll][4];
  unsigned sv[kMxUnroll];
#pragma unroll
  for (int u = 0; u < kMxUnroll; ++u) {
    if (FULL || u < cnt) {
      qv[u][0] = *reinterpret_cast<const u32x4*>(qp + u * kMxLine);
      qv[u][1] = *reinterpret_cast<const u32x4*>(qp + u * kMxLine + 16);
      sv[u] = *reinterpret_cast<const unsigned*>(sp + u * 4);
    }
  }
#pragma unroll
  for (int u = 0; u < kMxUnroll; ++u) {
#pragma unroll
    for (int j = 0; j < 4; ++j) xv[u][j] = u32x4{0u, 0u, 0u, 0u};
  }
  if (xok) {                                           // (one masked region for all of the wave's x loads)
#pragma unroll
    for (int u = 0; u < kMxUnroll; ++u) {
      if (FULL || u < cnt) {
#pragma unroll
        for (int j = 0; j < 4; ++j) xv[u][j] = *reinterpret_cast<const u32x4*>(xp + u * kMxLine + j * 8);
      }
    }
  }
#pragma unroll
  for (int u = 0; u < kMxUnroll; ++u) {
    if (FULL || u < cnt) {
      // e8m0 byte g of the line -> 2^(byte - 127) as f32 bits (the conversion reads the exponent field)
      const float scale = __uint_as_float(((sv[u] >> (8 * g)) & 0xffu) << 23);
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const unsigned c0 = qv[u][j >> 1][2 * (j & 1)], c1 = qv[u][j >> 1][2 * (j & 1) + 1];
        const u32x4 w = {mx_cvt2(c0, scale, false), mx_cvt2(c0, scale, true), mx_cvt2(c1, scale, false),
                         mx_cvt2(c1, scale, true)};
        acc = mfma16x16x32(__builtin_bit_cast(bf16x8, w), __builtin_bit_cast(bf16x8, xv[u][j]), acc);
      }
    }
  }
}

__global__ __launch_bounds__(kSkMaxWaves * 64)
void skinny_mx_kernel(const SkinnyMxArgs a) {
  extern __shared__ f32x4 part[];                      // [W][64], dynamic: none for a one-wave block
  const int lane = threadIdx.x & 63, g = lane >> 4, r16 = lane & 15;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int W = (int)(blockDim.x >> 6);
  const int n0 = blockIdx.x * kSkCols;

  const int lines = a.K >> 7;
  const int lgw = __builtin_ctz((unsigned)W);          // W is a power of two (the launcher)
  const int l0 = (wave * lines) >> lgw, l1 = ((wave + 1) * lines) >> lgw;

  int nrow = n0 + r16;
  nrow = nrow < a.e.N ? nrow : a.e.N - 1;             // the tail group: clamped for the loads, not stored
  const bool xok = r16 < a.e.M;
  const unsigned char* qp = a.q + (long)nrow * a.ldq + (long)l0 * kMxLine + 32 * g;
  const unsigned char* sp = a.s + (long)nrow * a.lds + (long)l0 * 4;
  const bf16_t* xp = a.x + (long)(xok ? r16 : 0) * a.lda + (long)l0 * kMxLine + 32 * g;

  f32x4 acc = {0.f, 0.f, 0.f, 0.f};
  for (int l = l0; l < l1; l += kMxUnroll) {
    const int cnt = l1 - l;                            // (wave-uniform)
    if (cnt >= kMxUnroll) skinny_mx_lines<true>(qp, sp, xp, xok, g, kMxUnroll, acc);
    else skinny_mx_lines<false>(qp, sp, xp, xok, g, cnt, acc);
    qp += kMxUnroll * kMxLine;
    sp += kMxUnroll * 4;
    xp += kMxUnroll * kMxLine;
  }

  if (!skinny_reduce(part, acc, wave, lane, W)) return;    // in wave order
  skinny_epilogue(a.e, acc, r16, n0 + 4 * g);
}

inline bool mx_shape_ok(int M, int N, int K) {
  return M >= 1 && M <= kSkMaxM && N >= 8 && N % 8 == 0 && K >= kMxLine && K % kMxLine == 0;
}

// the pure plan: (waves per block, blocks) of a shape on `cus` compute units (the head of the file)
inline void skinny_mx_plan(int N, int K, int cus, int* waves, int* blocks) {
  const long nb = ((long)N + kSkCols - 1) / kSkCols;
  const int lines = K / kMxLine;
  const long want = ((long)kSkWavesPerCu * cus + nb - 1) / nb;
  int w = 1;
  while (w < kSkMaxWaves && w < want) w *= 2;          // pow2ceil(want), at most 16
  while (w > lines) w /= 2;                            // at most pow2floor(lines)
  *waves = w < 1 ? 1 : w;
  *blocks = (int)nb;
}

// "skinny_mx<W,out[,bias][,relu][,res]>"
const char* skinny_mx_name(int waves, int flags) {
  static const std::string* table = sk_make_names("skinny_mx");
  return sk_name(table, waves, flags);
}

}  // namespace

// out[0] = waves per block, out[1] = blocks of (M, N, K) on a device of `cus` compute units: pure.
// hipErrorInvalidValue for a shape outside 1 <= M <= 16, K % 128 == 0, N % 8 == 0.
LJS_API int ljs_skinny_mx_plan(int M, int N, int K, int cus, int* out) {
  if (!mx_shape_ok(M, N, K) || cus < 1 || !out) return (int)hipErrorInvalidValue;
  skinny_mx_plan(N, K, cus, out, out + 1);
  return 0;
}

// y [M][N] (ldc) = epi(x [M][K] (lda) . W_hat^T), W_hat from the codes q [N][K] (ldq, bytes) and the scale
// bytes s [N][K / 32] (lds): the head of the file.  bias, res and the flags as ljs_skinny_bf16 takes them.
// Returns hipErrorInvalidValue, and launches and records nothing, for a shape outside the bounds, a null
// x / q / s / y, leading dimensions below the row length, rows of x or q that are not 16-byte aligned, scale
// rows that are not 4-byte aligned, y or res not aligned to a lane's 4 values, a misaligned bias, or a
// residual with an f32 output.
LJS_API int ljs_skinny_mx(const void* x, const void* q, const void* s, void* y, const void* bias, const void* res,
                          int M, int N, int K, long lda, long ldq, long lds, long ldc, long res_ld, int out_f32,
                          int bias_f32, int res_f32, int relu, hipStream_t st) {
  if (!mx_shape_ok(M, N, K) || !x || !q || !s) return (int)hipErrorInvalidValue;
  if (lda < K || ldq < K || lds < K / 32 || lda % 8 || ldq % 16 || lds % 4 || (((uintptr_t)x) & 15u) ||
      (((uintptr_t)q) & 15u) || (((uintptr_t)s) & 3u))
    return (int)hipErrorInvalidValue;
  if (!sk_epi_ok(y, bias, res, N, ldc, res_ld, out_f32, bias_f32, res_f32)) return (int)hipErrorInvalidValue;
  SkinnyMxArgs a{};
  a.x = (const bf16_t*)x;
  a.q = (const unsigned char*)q;
  a.s = (const unsigned char*)s;
  a.e = SkinnyEpi{y, bias, res, ldc, res_ld, M, N, sk_epi_flags(bias, res, out_f32, bias_f32, res_f32, relu)};
  a.lda = lda; a.ldq = ldq; a.lds = lds;
  a.K = K;
  int waves, blocks;
  skinny_mx_plan(N, K, ljs_device_cus(), &waves, &blocks);
  if (ljs_skinny_forced_waves() > 0) waves = ljs_skinny_forced_waves();
  const dim3 grid((unsigned)blocks);
  const size_t lds_bytes = waves > 1 ? (size_t)waves * 64 * sizeof(f32x4) : 0;
  hipLaunchKernelGGL(skinny_mx_kernel, grid, dim3((unsigned)waves * 64), lds_bytes, st, a);
  const int rc = (int)hipGetLastError();
  if (rc == 0) ljs_launch_rec(skinny_mx_name(waves, a.e.flags), grid, (unsigned)waves * 64);   // a failed launch leaves no record
  return rc;
}
