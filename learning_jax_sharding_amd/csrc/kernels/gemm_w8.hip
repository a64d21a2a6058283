// Tile GEMM on MX-fp8 weights (W8A16): y[m][n] = epi(sum_k x[m][k] W_hat[n][k]) for ANY M >= 1 rows of bf16
// activations, K % 128 == 0, N % 8 == 0, with
//     W_hat[n][k] = e4m3(q[n][k]) * 2^(s[n][k / 32] - 127),
// the "QT" shadow skinny_mx.hip streams for M <= 16 (e4m3 codes [N][K], row stride ldq; e8m0 scale bytes
// [N][K / 32], row stride lds).  x is never quantised and W_hat never exists as bf16 in memory: the B operand
// is dequantised on its way into LDS.  W_hat is an exact bf16 value, so the result is the bf16 tile GEMM's
// (gemm.hip, gemm_lean_kernel at the 128x128 tile) on the dequantised weight, bit for bit: the fragment-to-k
// mapping, the k-step order and the swapped MFMA operands are that kernel's.  Forward only, no split-K.
//
// Block: 4 waves (2 x 2), BM x 128 output tile with BM = 128 (64x64 wave tiles) or 64 (32x64), K-tile 64, two
// ring stages of (A image, B image): 64 KiB at BM = 128, two blocks per CU.
//   A (x)   LDS-DMA into gemm.hip's XOR-swizzled [BM][64] bf16 image: DmaTile<BM, true, 4> pieces through a
//           descriptor that ends at row M - 1 (a lane whose row is past M gets an out-of-range offset as
//           well, so it reads zeros whichever offsets the range check adds up).
//   B (W)   thread t owns row t >> 1, MX block t & 1 of the K-tile: two 16-byte buffer loads of codes and one
//           scale byte, through descriptors that end at row N - 1 (a row past N: an out-of-range offset,
//           zeros).  16 v_cvt_scalef32_pk_bf16_fp8 turn the 32 codes into 32 bf16 and four swizzled
//           ds_write_b128 put them where an LDS-DMA of the bf16 weight would have: the fragment reads are
//           frag<128, true>, unchanged.  (prefill128.hip's MX path, applied to a GEMM operand.)
//           The scale is one byte per (row, K-tile half); a dword per two K-tiles would save a load in every
//           other tile and cost a register and a tile-parity select: not taken, the byte rides with the codes.
// One barrier per K-tile.  At the top of tile f: vmcnt(0) -- the only vector-memory operations in flight are
// this wave's A pieces of f, the B loads of f were consumed by their conversions, so the counted wait's count
// is 0 -- and lgkmcnt(0) (this thread's B writes of f), then the barrier; then the A DMA and the B loads of
// f + 1 are issued (into the stage every wave has finished reading), then k-steps 0 and 1 of f, then the
// conversions and writes of f + 1's B.  The first tile's A and B are staged before the loop.
//
// One block per output tile, XCD-remapped, M-tiles fastest within a 128-column panel: the blocks that share a
// [128][K] code panel run together, so the panel comes from HBM once and from L2 afterwards.  No atomics,
// workspace, memset or tickets: nothing to re-arm for a graph replay.
//
// Epilogue, the skinny kernels' order: + bias (f32 or bf16) in f32, ReLU, one rounding to bf16 or f32, then
// bf16(bf16(y) + bf16(res)) for a bf16 or f32 residual (bf16 output only).  bf16 output: the text of
// gemm_epi_bf16.h, stated once for all tile GEMMs; f32 output: 16-byte stores of a lane's 4 columns.
//
// The plan (ljs_gemm_w8_plan) is pure: 64 rows when M <= 64 or when 128-row tiles would leave CUs without a
// block (ceil(M / 128) ceil(N / 128) < cus), else 128.  ljs_gemm_w8_set_rows forces the rows (tests).
// Measured figures: profiles/PERF_NOTES.md ("W8A16 tile GEMM").
#include "gemm_tile.h"
#include "skinny_common.h"
#include <stdio.h>

namespace {

constexpr int kW8BN = 128;

struct W8Args {
  GemmArgs p;                          // x as A, y as C, bias, res, M / N / K, flags: what the epilogue text reads
  const unsigned char *q, *s;
  long ldq, lds;
};

template <int BM, bool OUT_F32, int RES>
__global__ __launch_bounds__(256, 2) void gemm_w8_kernel(const W8Args a) {
  constexpr int BN = kW8BN, WM = 2, WN = 2, NW = 4, NST = 2;
  constexpr int TM = BM / WM / 16, TN = BN / WN / 16;
  constexpr int A_TILE = BM * BK, B_TILE = BN * BK, STAGE = A_TILE + B_TILE;
  [[maybe_unused]] constexpr bool PLAIN = false, NOALPHA = true, HAS_R = RES == 1 || RES == 2;
  static_assert(!OUT_F32 || RES == 0, "a residual takes a bf16 output");
  using TA = DmaTile<BM, true, NW>;
  __shared__ __attribute__((aligned(16))) bf16_t smem[NST * STAGE];

  const GemmArgs& p = a.p;
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wr = wave / WN, wc = wave % WN;
  const int ntm = (p.M + BM - 1) / BM;
  const int G = gridDim.x;                             // ntm * ceil(N / 128): one block per tile
  const int slot = xcd_remap(blockIdx.x, G);
  const int tm_i = slot % ntm, tn_i = slot / ntm;      // M-tiles fastest within a column panel
  const int nk = p.K / BK;

  // ---- A: DMA pieces; a lane whose row is past M reads zeros
  const __amdgpu_buffer_rsrc_t ra = make_rsrc(p.A, 2 * ((long)(p.M - 1) * p.lda + p.K));
  int a_off = __builtin_amdgcn_readfirstlane((int)((long)tm_i * BM * p.lda * 2));
  TA ta;
  ta.init(p.lda, wave, lane);
#pragma unroll
  for (int i = 0; i < TA::PER_WAVE; ++i)
    if (tm_i * BM + 8 * (wave + NW * i) + (lane >> 3) >= p.M) ta.voff[i] = 0x7ffffff0;

  // ---- B: this thread's row and MX block of every K-tile
  const int brow = tid >> 1, bh = tid & 1;
  const int bn = tn_i * BN + brow;
  const bool bok = bn < p.N;
  const __amdgpu_buffer_rsrc_t rq = make_rsrc(a.q, (long)(p.N - 1) * a.ldq + p.K);
  const __amdgpu_buffer_rsrc_t rs = make_rsrc(a.s, (long)(p.N - 1) * a.lds + p.K / 32);
  const int q_off = bok ? (int)((long)bn * a.ldq) + 32 * bh : 0;
  const int s_off = bok ? (int)((long)bn * a.lds) + bh : 0;
  u32x4 cq[2];
  unsigned sc;
  auto load_b = [&](int kt) {
    const int o = bok ? q_off + kt * BK : 0x7ffffff0;
    cq[0] = __builtin_amdgcn_raw_buffer_load_b128(rq, o, 0, 0);
    cq[1] = __builtin_amdgcn_raw_buffer_load_b128(rq, bok ? o + 16 : o, 0, 0);
    sc = (unsigned)__builtin_amdgcn_raw_buffer_load_b8(rs, bok ? s_off + kt * 2 : 0x7ffffff0, 0, 0) & 0xffu;
  };
  auto put_b = [&](bf16_t* Bs) {
    // e8m0 byte -> 2^(byte - 127) as f32 bits (the conversion reads the exponent field)
    const float sf = __uint_as_float(sc << 23);
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      unsigned w[8];
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        w[2 * j] = __builtin_bit_cast(unsigned, __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(cq[i][j], sf, false));
        w[2 * j + 1] = __builtin_bit_cast(unsigned, __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(cq[i][j], sf, true));
      }
      const int kc = 4 * bh + 2 * i;                   // 16-byte chunks kc, kc + 1 of the row's 8
      *reinterpret_cast<u32x4*>(Bs + brow * BK + swz_k(brow, kc) * 8) = u32x4{w[0], w[1], w[2], w[3]};
      *reinterpret_cast<u32x4*>(Bs + brow * BK + swz_k(brow, kc + 1) * 8) = u32x4{w[4], w[5], w[6], w[7]};
    }
  };

  f32x4 acc[TM][TN];
#pragma unroll
  for (int i = 0; i < TM; ++i)
#pragma unroll
    for (int j = 0; j < TN; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};

  bf16x8 ka[TM], kb[TN], la[TM], lb[TN];
  auto read_frags = [&](const bf16_t* As_, int ks, bf16x8* af, bf16x8* bfr) {
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

  // ---- tile 0 into stage 0
  ta.issue(ra, smem, a_off, wave);
  load_b(0);
  put_b(smem + A_TILE);

  for (int f = 0; f < nk; ++f) {
    bf16_t* cur = smem + (f & 1) * STAGE;
    bf16_t* nxt = smem + ((f + 1) & 1) * STAGE;
    asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");   // A pieces of f landed, B writes of f done
    __builtin_amdgcn_s_barrier();                       // ... for every wave; every read of tile f - 1 done
    asm volatile("" ::: "memory");
    const bool more = f + 1 < nk;
    if (more) {
      a_off += BK * 2;
      ta.issue(ra, nxt, a_off, wave);
      load_b(f + 1);
    }
    read_frags(cur, 0, ka, kb);
    read_frags(cur, 1, la, lb);
    mfmas(ka, kb);
    mfmas(la, lb);
    if (more) put_b(nxt + A_TILE);
  }

  // ------------------------------------------------------------ epilogue
  const bool relu = p.flags & 1, has_bias = p.flags & 2, bias_f32 = p.flags & 4;
  const __amdgpu_buffer_rsrc_t rc = make_rsrc(p.C, (OUT_F32 ? 4 : 2) * ((long)(p.M - 1) * p.ldc + p.N));
  const int m0 = tm_i * BM + wr * (BM / WM), n0 = tn_i * BN + wc * (BN / WN);
  const int g = lane >> 4;
  if constexpr (!OUT_F32) {
    [[maybe_unused]] const WorkItem w{0, tm_i, tn_i, 0, 0};
    [[maybe_unused]] const int it = 0;
    constexpr bool st_sc1 = false, psum_on = false;
    [[maybe_unused]] float tsum = 0.f;
#include "gemm_epi_bf16.h"
  } else {
    // the lane holds C[m0 + 16 ii + (lane & 15)][n0 + 16 j + 4 g + 0..3]; N % 8 == 0: its 4 columns are whole
#pragma unroll
    for (int j = 0; j < TN; ++j) {
      const int col = n0 + j * 16 + 4 * g;
      float bv[4] = {0.f, 0.f, 0.f, 0.f};
      if (has_bias && col < p.N) {
#pragma unroll
        for (int e = 0; e < 4; ++e)
          bv[e] = bias_f32 ? reinterpret_cast<const float*>(p.bias)[col + e]
                           : bf2f(reinterpret_cast<const bf16_t*>(p.bias)[col + e]);
      }
#pragma unroll
      for (int ii = 0; ii < TM; ++ii) {
        const int row = m0 + ii * 16 + (lane & 15);
        f32x4 v;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          v[e] = acc[ii][j][e] + bv[e];
          if (relu) v[e] = fmaxf(v[e], 0.f);
        }
        const bool ok = row < p.M && col < p.N;
        const int off = ok ? (int)(((long)row * p.ldc + col) * 4) : 0x7ffffff0;
        __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u32x4, v), rc, off, 0, 0);
      }
    }
  }
}

// the explicit instances: (rows, output, epilogue operand); bias and ReLU are run-time flags, as in gemm.hip
#define LJS_W8_INST(BM)                                                                    \
  template __global__ void gemm_w8_kernel<BM, false, 0>(const W8Args);                     \
  template __global__ void gemm_w8_kernel<BM, false, 1>(const W8Args);                     \
  template __global__ void gemm_w8_kernel<BM, false, 2>(const W8Args);                     \
  template __global__ void gemm_w8_kernel<BM, true, 0>(const W8Args);
LJS_W8_INST(128)
LJS_W8_INST(64)
#undef LJS_W8_INST

int g_w8_rows = 0;                       // > 0: the rows forced by tests (ljs_gemm_w8_set_rows)

inline bool w8_shape_ok(int M, int N, int K) {
  return M >= 1 && N >= 8 && N % 8 == 0 && K >= 128 && K % 128 == 0;
}

// the pure plan: rows of the block tile and blocks of a shape on `cus` compute units (the head of the file)
inline void w8_plan(int M, int N, int K, int cus, int* rows, int* blocks) {
  (void)K;
  const long ntn = ((long)N + kW8BN - 1) / kW8BN;
  const long t128 = (((long)M + 127) / 128) * ntn;
  const int r = (M <= 64 || t128 < cus) ? 64 : 128;
  *rows = r;
  *blocks = (int)((((long)M + r - 1) / r) * ntn);
}

// "gemm_w8<R128|R64,bf16|f32[,bias][,relu][,res]>"
const char* w8_name(int rows, int flags) {
  struct Name { char s[48]; };
  static const Name* table = [] {
    auto* t = new Name[2 * 16];
    for (int r = 0; r < 2; ++r)
      for (int f = 0; f < 16; ++f)
        snprintf(t[r * 16 + f].s, sizeof(t[0].s), "gemm_w8<R%d,%s%s%s%s>", r ? 64 : 128, f & 1 ? "f32" : "bf16",
                 f & 2 ? ",bias" : "", f & 4 ? ",relu" : "", f & 8 ? ",res" : "");
    return t;
  }();
  const int f = (flags & kSkOutF32 ? 1 : 0) | (flags & kSkBias ? 2 : 0) | (flags & kSkRelu ? 4 : 0) |
                (flags & kSkRes ? 8 : 0);
  return table[(rows == 64 ? 16 : 0) + f].s;
}

template <int BM>
void w8_launch(const W8Args& a, int flags, dim3 grid, hipStream_t st) {
  if (flags & kSkOutF32) hipLaunchKernelGGL((gemm_w8_kernel<BM, true, 0>), grid, dim3(256), 0, st, a);
  else if (!(flags & kSkRes)) hipLaunchKernelGGL((gemm_w8_kernel<BM, false, 0>), grid, dim3(256), 0, st, a);
  else if (flags & kSkResF32) hipLaunchKernelGGL((gemm_w8_kernel<BM, false, 2>), grid, dim3(256), 0, st, a);
  else hipLaunchKernelGGL((gemm_w8_kernel<BM, false, 1>), grid, dim3(256), 0, st, a);
}

}  // namespace

// Tests: force the block tile's rows (64 or 128); 0 restores the plan.
LJS_API int ljs_gemm_w8_set_rows(int rows) {
  if (rows != 0 && rows != 64 && rows != 128) return (int)hipErrorInvalidValue;
  g_w8_rows = rows;
  return 0;
}

// out[0] = rows of the block tile (64 or 128), out[1] = blocks of (M, N, K) on a device of `cus` compute
// units: pure (a forced row count does not enter).  hipErrorInvalidValue for a shape outside M >= 1,
// K % 128 == 0, N % 8 == 0.
LJS_API int ljs_gemm_w8_plan(int M, int N, int K, int cus, int* out) {
  if (!w8_shape_ok(M, N, K) || cus < 1 || !out) return (int)hipErrorInvalidValue;
  w8_plan(M, N, K, cus, out, out + 1);
  return 0;
}

// y [M][N] (ldc) = epi(x [M][K] (lda) . W_hat^T), ljs_skinny_mx's operands and argument order for any M >= 1.
// Returns hipErrorInvalidValue, and launches and records nothing, for what ljs_skinny_mx refuses (but for
// M > 16) and for an operand whose last byte offset does not fit 31 bits.
LJS_API int ljs_gemm_w8(const void* x, const void* q, const void* s, void* y, const void* bias, const void* res,
                        int M, int N, int K, long lda, long ldq, long lds, long ldc, long res_ld, int out_f32,
                        int bias_f32, int res_f32, int relu, hipStream_t st) {
  if (!w8_shape_ok(M, N, K) || !x || !q || !s) return (int)hipErrorInvalidValue;
  if (lda < K || ldq < K || lds < K / 32 || lda % 8 || ldq % 16 || lds % 4 || (((uintptr_t)x) & 15u) ||
      (((uintptr_t)q) & 15u) || (((uintptr_t)s) & 3u))
    return (int)hipErrorInvalidValue;
  if (!sk_epi_ok(y, bias, res, N, ldc, res_ld, out_f32, bias_f32, res_f32)) return (int)hipErrorInvalidValue;
  int rows, blocks;
  w8_plan(M, N, K, ljs_device_cus(), &rows, &blocks);
  if (g_w8_rows > 0) {
    rows = g_w8_rows;
    blocks = (int)((((long)M + rows - 1) / rows) * (((long)N + kW8BN - 1) / kW8BN));
  }
  // every byte offset a lane forms stays below 2^31 (x: up to the last row of the last, partial, tile)
  const long lim = 0x7fffffffL;
  const long mpad = (((long)M + rows - 1) / rows) * rows;
  if ((mpad * lda + K) * 2 > lim || (long)N * ldq + K > lim || ((long)M * ldc + N) * (out_f32 ? 4 : 2) > lim ||
      (res && ((long)M * res_ld + N) * (res_f32 ? 4 : 2) > lim))
    return (int)hipErrorInvalidValue;
  const int flags = sk_epi_flags(bias, res, out_f32, bias_f32, res_f32, relu);
  W8Args a{};
  a.p.A = (const bf16_t*)x;
  a.p.C = y;
  a.p.bias = bias;
  a.p.res = res;
  a.p.lda = lda; a.p.ldc = ldc; a.p.ldr = res_ld;
  a.p.M = M; a.p.N = N; a.p.K = K;
  a.p.batch = 1; a.p.splitk = 1; a.p.kt_per_split = K / BK;
  a.p.alpha = 1.f;
  a.p.flags = (relu ? 1 : 0) | (bias ? 2 : 0) | (bias && bias_f32 ? 4 : 0) | (res ? kResAdd : 0) |
              (res && res_f32 ? kResF32 : 0);
  a.q = (const unsigned char*)q;
  a.s = (const unsigned char*)s;
  a.ldq = ldq; a.lds = lds;
  const dim3 grid((unsigned)blocks);
  if (rows == 64) w8_launch<64>(a, flags, grid, st);
  else w8_launch<128>(a, flags, grid, st);
  const int rc = (int)hipGetLastError();
  if (rc == 0) ljs_launch_rec(w8_name(rows, flags), grid, 256);   // a failed launch leaves no record
  return rc;
}
