// LJS_HIPCC_FLAGS: -Xclang -target-feature -Xclang -packed-fp32-ops -mllvm -amdgpu-mfma-vgpr-form
// Chunked prefill at head dim 128: flash-style MFMA attention of T >= 1 new positions per sequence over the
// KV cache buffers themselves (bf16 q and o; bf16 or MX-fp8 caches).  prefill.hip is the head dim 64 file;
// the semantics, the row mapping and the rounding points are exactly its own (ops/kernels.py,
// attn_chunk_reference): q is (B, T, H, 128), kc / vc are (B, cap, Hkv, 128), lens is int32 [B] ON THE
// DEVICE, and row (b, t, h) attends to the cache rows [0, n), n = clamp(lens[b] + t + 1, 0, cap), of
// key/value head h / G:
//     o[b][t][h]    = bf16( sum_key bf16(p[key]) vc[b][key][h / G] / l ),  p = exp2(s scale log2e - m)
//     lse2[b][t][h] = m + log2(l)
// n = 0 gives o = 0, lse2 = +inf.  No kernel argument depends on lens: a captured launch follows it.
//
// Rows and grid: prefill.hip's.  A row is a (t, g) pair of one (batch, key/value head), r = t G + g, G in
// 1..16; a block of 4 waves takes ROWS consecutive rows, 128 (two 16-row MFMA chains per wave that share
// every K and V fragment) or 64 (one chain); the grid is (row tiles, Hkv, B), the latest positions first.
//
// What is new at 128 (256-byte rows: prefill.hip's [64][64] image, its swizzle and its 128-byte output
// rows do not carry over):
//   * LDS.  K and V tiles of 64 keys are [64][128] bf16 images, 16-byte chunk c of row r at c ^ swz(r),
//     attention128.hip's swizzle: conflict-free for the ds_read_b128 operand columns and for the
//     transposing ds_read_b64_tr_b16 reads.  Two stages of (K, V), 64 KiB, one barrier per tile, two blocks
//     per CU.  bf16 tiles arrive by LDS-DMA (16 pieces of 4 rows, four per wave) with the swizzle on the
//     source address, through a descriptor rebased per tile that ends with the block's last live row:
//     rows past it land as zeros whatever the memory holds.
//   * Registers.  S^T = K . Q^T with the 16x16x32 bf16 MFMA, four k-steps per 16-key sub-tile; Q fragments
//     go from global memory straight to VGPRs (four u32x4 per chain); a lane owns one row, so the row's
//     key limit is one compare applied by a select in front of the raw exp2, and the softmax is in-lane
//     but for the row-of-4 max and sum; O^T is eight f32x4 per chain; the O rescale is skipped
//     wave-uniformly when no running max moved.  A wave runs nothing beyond the largest limit of its rows,
//     and the selects only over the boundary band above its smallest limit: a wave-uniform branch inside
//     ONE tile body (chunk_tile says why it is not prefill.hip's two bodies).
//   * MX-fp8 cache (e4m3 bytes (B, cap, Hkv, 128), e8m0 scales (B, cap, Hkv, 4), strides in bytes): a row is
//     four scale blocks; thread tid takes row tid >> 2, block tid & 3: 32 bytes of K, 32 of V and one scale
//     byte each of the NEXT tile into VGPRs while the current tile computes, converted with the scaled
//     conversion (exact) into four swizzled 16-byte chunks per tensor by ds_write_b128.  From the image on
//     the sweep is the bf16 instance's: attn_chunk_q8 has the bits of attn_chunk on the dequantised cache.
//   * Output.  After the sweep a wave stages its rows in its own part of the idle ring (8 KiB at 128 rows,
//     4 KiB at 64) and they leave as whole 256-byte rows, four rows per 16-byte-per-lane store.  No
//     atomics, no memset, no workspace, no tickets; the same bits on every run.
//
// The plan (128-row tiles, 64 when a group's rows fit one or 128-row tiles would leave CUs idle) is
// prefill.hip's exported ljs_chunk_plan, and ljs_chunk_set_rows forces both files' tiles.
#include "cache_common.h"
#include "common.h"

LJS_API int ljs_chunk_plan(int B, int T, int H, int Hkv, int cus, int* out);
LJS_API int ljs_chunk_get_rows();

namespace {

constexpr int kD = 128;                 // head dim
constexpr int kKeys = 64;               // keys per tile
constexpr int kImg = kKeys * kD;        // elements of one LDS image (16 KiB)
constexpr int kThreads = 256;
constexpr int kMaxG = 16;
constexpr float kLog2e = 1.4426950408889634f;

struct Chunk128Args {
  const bf16_t* q;
  const unsigned char *kc, *vc;         // bf16 rows, or e4m3 bytes (MX8)
  const unsigned char *ksc, *vsc;       // MX8: the e8m0 scales
  bf16_t* o;
  float* lse;                           // [B][T][H]
  const int* lens;
  long qb, qt, qh, ob, ot, oh;          // elements
  long kb, ks, kh, vb, vs, vh;          // BYTES (both cache kinds)
  long ksb, kss, ksh, vsb, vss, vsh;    // bytes
  int T, H, G, cap;
  float scale_log2;
};

__device__ __forceinline__ float exp2_raw(float x) { return __builtin_amdgcn_exp2f(x); }

// ---- the LDS image (attention128.hip's): element index of 16-byte chunk c16 / 8-byte piece c8 of a row.  swz's
// bits (3..0) are (r2 ^ r3, r1, r0, r2) of the row number.
__device__ __forceinline__ int swz(int row) {
  return ((row & 3) << 1) | ((row >> 2) & 1) | ((((row >> 2) ^ (row >> 3)) & 1) << 3);
}
__device__ __forceinline__ int img16(int row, int c16) { return row * kD + ((c16 ^ swz(row)) << 3); }
__device__ __forceinline__ int img8(int row, int c8) { return img16(row, c8 >> 1) + ((c8 & 1) << 2); }

// The lane parts of the fragment addresses, once per kernel: the swizzle reads the row number's low four
// bits only, so a row base that is a multiple of 16 is an immediate offset on top of them.
struct LaneOff {
  int rows[4];   // img16(lane & 15, 4 ks + (lane >> 4)): the ds_read_b128 operand of k-step ks
  int tr[8];     // img8(4 (lane >> 4) + ((lane & 15) >> 2), 4 dt + (lane & 3)): the transposed operand of d tile dt
};
__device__ __forceinline__ LaneOff lane_off(int lane) {
  LaneOff f;
  const int i = lane & 15, g = lane >> 4;
#pragma unroll
  for (int ks = 0; ks < 4; ++ks) f.rows[ks] = img16(i, 4 * ks + g);
#pragma unroll
  for (int dt = 0; dt < 8; ++dt) f.tr[dt] = img8(4 * g + (i >> 2), 4 * dt + (i & 3));
  return f;
}
// A operand K[m = key 16 jt + (lane & 15)][k = d 32 ks + 8 (lane >> 4) ..]
__device__ __forceinline__ bf16x8 frag_k(const bf16_t* img, int jt, int ks, const LaneOff& f) {
  return __builtin_bit_cast(bf16x8, *reinterpret_cast<const u32x4*>(img + 16 * jt * kD + f.rows[ks]));
}
// A operand V^T[m = d 16 dt + (lane & 15)][k = key]: elements 0..3 keys R0 + 4 g + 0..3, elements 4..7 keys
// R0 + 16 + 4 g + 0..3 (the order of the two accumulator tiles P comes from)
__device__ __forceinline__ bf16x8 frag_vt(const bf16_t* img, int R0, int dt, const LaneOff& f) {
  return join_bf16x8(lds_read_tr16(img + R0 * kD + f.tr[dt]), lds_read_tr16(img + (R0 + 16) * kD + f.tr[dt]));
}

struct RowState {
  f32x4 o[8];    // O^T: d 16 dt + 4 (lane >> 4) + e of row lane & 15
  float m, l;    // the running max (all 4 lanes of a row agree) and this lane's part of the sum
};

// One 64-key tile for a wave's CH chains of 16 rows.  mask (wave-uniform): a score whose key is at or beyond
// its row's limit nr[c] is replaced by -inf before anything reads it.  ONE body with a branch around the
// selects, not prefill.hip's two instantiations: with both inlined the 128-row instances spilled (85
// VGPRs bf16, 95 MX-fp8; profiles/chunk128/resources.txt).
template <int CH>
__device__ __forceinline__ void chunk_tile(RowState (&st)[CH], const bf16_t* Kt, const bf16_t* Vt,
                                           const bf16x8 (&qf)[CH][4], const int (&nr)[CH], int kbase, float sl2,
                                           bool mask, int lane, const LaneOff& f) {
  const int g = lane >> 4;
  f32x4 s[CH][4];
#pragma unroll
  for (int jt = 0; jt < 4; ++jt) {
#pragma unroll
    for (int c = 0; c < CH; ++c) s[c][jt] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int ks = 0; ks < 4; ++ks) {
      const bf16x8 kf = frag_k(Kt, jt, ks, f);
#pragma unroll
      for (int c = 0; c < CH; ++c) s[c][jt] = mfma16x16x32(kf, qf[c][ks], s[c][jt]);
    }
  }
  u32x4 pb[CH][2];
#pragma unroll
  for (int c = 0; c < CH; ++c) {
    if (mask) {
#pragma unroll
      for (int jt = 0; jt < 4; ++jt)
#pragma unroll
        for (int e = 0; e < 4; ++e) s[c][jt][e] = kbase + 16 * jt + 4 * g + e < nr[c] ? s[c][jt][e] : -INFINITY;
    }
    float tmax = fmaxf(fmaxf(s[c][0][0], s[c][0][1]), fmaxf(s[c][0][2], s[c][0][3]));
#pragma unroll
    for (int jt = 1; jt < 4; ++jt)
      tmax = fmaxf(tmax, fmaxf(fmaxf(s[c][jt][0], s[c][jt][1]), fmaxf(s[c][jt][2], s[c][jt][3])));
    tmax = row4_max(tmax);
    // scores are compared raw (scale > 0 keeps the order); the scale is one FMA in front of v_exp_f32
    const float m_new = fmaxf(st[c].m, tmax * sl2);
    const float m_use = m_new == -INFINITY ? 0.f : m_new;   // no key seen so far: p = 0
    const float alpha = exp2_raw(st[c].m - m_use);
    float ps0 = 0.f, ps1 = 0.f;
#pragma unroll
    for (int jt = 0; jt < 4; ++jt)
#pragma unroll
      for (int e = 0; e < 4; e += 2) {
        const float p0 = exp2_raw(fmaf(s[c][jt][e], sl2, -m_use));
        const float p1 = exp2_raw(fmaf(s[c][jt][e + 1], sl2, -m_use));
        s[c][jt][e] = p0;
        s[c][jt][e + 1] = p1;
        ps0 += p0;
        ps1 += p1;
      }
    // no lane's running max moved (the usual case after the first tiles): alpha is exactly 1, or the
    // row has seen no key and O is 0, so the O rescale is skipped wave-uniformly
    const bool rescale = !__all(m_new == st[c].m);
    st[c].l = st[c].l * alpha + (ps0 + ps1);
    st[c].m = m_new;
    if (rescale) {
#pragma unroll
      for (int dt = 0; dt < 8; ++dt) st[c].o[dt] = st[c].o[dt] * alpha;
    }
#pragma unroll
    for (int s2 = 0; s2 < 2; ++s2) {
      pb[c][s2][0] = pack_bf16x2(s[c][2 * s2][0], s[c][2 * s2][1]);
      pb[c][s2][1] = pack_bf16x2(s[c][2 * s2][2], s[c][2 * s2][3]);
      pb[c][s2][2] = pack_bf16x2(s[c][2 * s2 + 1][0], s[c][2 * s2 + 1][1]);
      pb[c][s2][3] = pack_bf16x2(s[c][2 * s2 + 1][2], s[c][2 * s2 + 1][3]);
    }
  }
#pragma unroll
  for (int s2 = 0; s2 < 2; ++s2)
#pragma unroll
    for (int dt = 0; dt < 8; ++dt) {
      const bf16x8 va = frag_vt(Vt, 32 * s2, dt, f);
#pragma unroll
      for (int c = 0; c < CH; ++c) st[c].o[dt] = mfma16x16x32(va, __builtin_bit_cast(bf16x8, pb[c][s2]), st[c].o[dt]);
    }
}

// bf16 cache: rows kb0 .. kb0 + 63 of one (batch, key/value head) slab into an image by LDS-DMA, 16 pieces
// of 4 rows x 256 bytes, four per wave.  The resource is rebased on the tile and ends with live row n_end
// - 1: rows at and beyond n_end land as zeros.  ld: the row stride in bytes.
__device__ __forceinline__ void dma_tile(const unsigned char* base, long ld, int kb0, int n_end, bf16_t* img, int wave,
                                         int lane) {
  const int nr = n_end - kb0 < kKeys ? n_end - kb0 : kKeys;
  const u32x4 rs = rsrc_u4(base + (long)kb0 * ld, (long)(nr - 1) * ld + 2 * kD);
  const int ld32 = (int)ld;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int pc = wave + 4 * i, row = 4 * pc + (lane >> 4);
    const int c = (lane & 15) ^ swz(row);
    dma_lds_x4(rs, row < nr ? row * ld32 + c * 16 : 0x7ffffff0, img + pc * 512);
  }
}

// MX-fp8 cache: a lane's scale block (32 elements) of a row of K and of V, on its way from the descriptors
// (which end with the block's last live row) to the bf16 images
struct Q8Regs {
  u32x4 k[2], v[2];
  unsigned ke, ve;
  __device__ __forceinline__ void load(const __amdgpu_buffer_rsrc_t& rk, const __amdgpu_buffer_rsrc_t& rv,
                                       const __amdgpu_buffer_rsrc_t& rks, const __amdgpu_buffer_rsrc_t& rvs,
                                       const Chunk128Args& a, int kb0, int tid) {
    const int row = kb0 + (tid >> 2), blk = tid & 3;
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      k[i] = __builtin_amdgcn_raw_buffer_load_b128(rk, row * (int)a.ks + blk * 32 + 16 * i, 0, 0);
      v[i] = __builtin_amdgcn_raw_buffer_load_b128(rv, row * (int)a.vs + blk * 32 + 16 * i, 0, 0);
    }
    ke = __builtin_amdgcn_raw_buffer_load_b8(rks, row * (int)a.kss + blk, 0, 0);
    ve = __builtin_amdgcn_raw_buffer_load_b8(rvs, row * (int)a.vss + blk, 0, 0);
  }
  static __device__ __forceinline__ void put(bf16_t* img, const u32x4 (&x)[2], unsigned e, int tid) {
    // 2^(e - 127), as prefill.hip builds it: the conversion reads the exponent field (0: 2^-127).  kv_append128<..,mx8> never
    // writes 0xFF (mx_exponent stops at 127: byte 254) and writes 0x00 only for a block whose amax is at most 1.75 * 2^-119,
    // the all-zero block among them, whose bytes are 0 and give 0 under any scale.
    const float sf = __uint_as_float(e << 23);
    const int row = tid >> 2, blk = tid & 3;
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      unsigned w[8];
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        w[2 * j] = __builtin_bit_cast(unsigned, __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(x[i][j], sf, false));
        w[2 * j + 1] = __builtin_bit_cast(unsigned, __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(x[i][j], sf, true));
      }
      *reinterpret_cast<u32x4*>(img + img16(row, 4 * blk + 2 * i)) = u32x4{w[0], w[1], w[2], w[3]};
      *reinterpret_cast<u32x4*>(img + img16(row, 4 * blk + 2 * i + 1)) = u32x4{w[4], w[5], w[6], w[7]};
    }
  }
  __device__ __forceinline__ void store(bf16_t* stage, int tid) const {
    put(stage, k, ke, tid);
    put(stage + kImg, v, ve, tid);
  }
};

// A lane's 32 d-values (8 tiles of 4) of local row rbase + (lane & 15) into a wave-private [rows][128] bf16
// image (the same chunk swizzle), and NR staged rows out as whole 256-byte rows, 4 per store instruction;
// row r0 + i of the block is (t, g) = (r / G, r % G).
__device__ __forceinline__ void stage_rows(bf16_t* img, int rbase, const f32x4 (&acc)[8], float mul, int lane) {
  const int r = rbase + (lane & 15), g = lane >> 4;
#pragma unroll
  for (int dt = 0; dt < 8; ++dt) {
    u32x2 w;
    w[0] = pack_bf16x2(acc[dt][0] * mul, acc[dt][1] * mul);
    w[1] = pack_bf16x2(acc[dt][2] * mul, acc[dt][3] * mul);
    *reinterpret_cast<u32x2*>(img + img16(r, 2 * dt + (g >> 1)) + 4 * (g & 1)) = w;
  }
}
template <int NR>
__device__ __forceinline__ void flush_rows(const bf16_t* img, bf16_t* base, const Chunk128Args& a, int r0, int R, int h0,
                                           int lane) {
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");   // this wave's image writes are done (wave-private)
  u32x4 v[NR / 4];
#pragma unroll
  for (int i = 0; i < NR / 4; ++i) v[i] = *reinterpret_cast<const u32x4*>(img + img16(4 * i + (lane >> 4), lane & 15));
#pragma unroll
  for (int i = 0; i < NR / 4; ++i) {
    const int r = r0 + 4 * i + (lane >> 4);
    if (r < R) {
      const int t = r / a.G, g = r - t * a.G;
      *reinterpret_cast<u32x4*>(base + (long)t * a.ot + (long)(h0 + g) * a.oh + 8 * (lane & 15)) = v[i];
    }
  }
}

template <int ROWS, bool MX8>
__global__ __launch_bounds__(kThreads, 2) void attn_chunk128_kernel(const Chunk128Args a) {
  constexpr int CH = ROWS / 64;          // 16-row chains per wave
  constexpr int WR = 16 * CH;            // rows per wave
  __shared__ __attribute__((aligned(16))) bf16_t smem[4 * kImg];   // [stage][K | V]
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const LaneOff f = lane_off(lane);
  const int tile = gridDim.x - 1 - blockIdx.x, j = blockIdx.y, b = blockIdx.z;
  const int R = a.T * a.G, h0 = j * a.G;
  const long len = a.lens[b];
  auto limit = [&](int t) {              // keys row (t, .) sees
    const long n = len + t + 1;
    return (int)(n < 0 ? 0 : (n > a.cap ? (long)a.cap : n));
  };
  const int r0 = tile * ROWS;
  const int n_max = limit(((r0 + ROWS < R ? r0 + ROWS : R) - 1) / a.G);    // of the block's last row
  const int nkt = (n_max + kKeys - 1) / kKeys;
  // this wave's rows: the smallest and the largest limit (a wave without rows computes nothing)
  const int r0w = r0 + wave * WR;
  const bool wave_live = r0w < R;
  const int w_lo = wave_live ? limit(r0w / a.G) : 0;
  const int w_hi = wave_live ? limit(((r0w + WR < R ? r0w + WR : R) - 1) / a.G) : 0;

  bf16x8 qf[CH][4];
  RowState st[CH];
  int nr[CH], trow[CH], grow[CH];
  bool ok[CH];
#pragma unroll
  for (int c = 0; c < CH; ++c) {
    const int r = r0w + 16 * c + (lane & 15);
    ok[c] = r < R;
    trow[c] = ok[c] ? r / a.G : 0;
    grow[c] = ok[c] ? r - trow[c] * a.G : 0;
    nr[c] = ok[c] ? limit(trow[c]) : w_hi;         // (a row past the end: zeros in, nothing out)
    const bf16_t* qp = a.q + (long)b * a.qb + (long)trow[c] * a.qt + (long)(h0 + grow[c]) * a.qh + 8 * (lane >> 4);
#pragma unroll
    for (int ks = 0; ks < 4; ++ks)
      qf[c][ks] = __builtin_bit_cast(bf16x8, ok[c] ? *reinterpret_cast<const u32x4*>(qp + 32 * ks) : u32x4{0u, 0u, 0u, 0u});
#pragma unroll
    for (int i = 0; i < 8; ++i) st[c].o[i] = f32x4{0.f, 0.f, 0.f, 0.f};
    st[c].m = -INFINITY;
    st[c].l = 0.f;
  }

  const unsigned char* kbp = a.kc + (long)b * a.kb + (long)j * a.kh;
  const unsigned char* vbp = a.vc + (long)b * a.vb + (long)j * a.vh;
  // MX8: descriptors over the whole live range (a row is 128 bytes and 4 scale bytes)
  __amdgpu_buffer_rsrc_t rk, rv, rks, rvs;
  Q8Regs regs;
  if constexpr (MX8) {
    rk = make_rsrc(kbp, n_max > 0 ? (long)(n_max - 1) * a.ks + kD : 0);
    rv = make_rsrc(vbp, n_max > 0 ? (long)(n_max - 1) * a.vs + kD : 0);
    rks = make_rsrc(a.ksc + (long)b * a.ksb + (long)j * a.ksh, n_max > 0 ? (long)(n_max - 1) * a.kss + kD / 32 : 0);
    rvs = make_rsrc(a.vsc + (long)b * a.vsb + (long)j * a.vsh, n_max > 0 ? (long)(n_max - 1) * a.vss + kD / 32 : 0);
  }
  auto issue = [&](int kt) {             // bf16: tile kt on its way into its stage
    bf16_t* stg = smem + (kt & 1) * 2 * kImg;
    dma_tile(kbp, a.ks, kt * kKeys, n_max, stg, wave, lane);
    dma_tile(vbp, a.vs, kt * kKeys, n_max, stg + kImg, wave, lane);
  };
  if (nkt > 0) {
    if constexpr (MX8) {
      regs.load(rk, rv, rks, rvs, a, 0, tid);
      regs.store(smem, tid);
    } else {
      issue(0);
    }
  }
#pragma unroll 1
  for (int kt = 0; kt < nkt; ++kt) {
    // tile kt is in its stage, and every wave is done with tile kt - 1 (the other stage)
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    const bool more = kt + 1 < nkt;
    if (more) {
      if constexpr (MX8) regs.load(rk, rv, rks, rvs, a, (kt + 1) * kKeys, tid);
      else issue(kt + 1);
    }
    const bf16_t* Kt = smem + (kt & 1) * 2 * kImg;
    const int kbase = kt * kKeys;
    if (kbase < w_hi) chunk_tile<CH>(st, Kt, Kt + kImg, qf, nr, kbase, a.scale_log2, kbase + kKeys > w_lo, lane, f);
    if constexpr (MX8) {
      if (more) regs.store(smem + ((kt + 1) & 1) * 2 * kImg, tid);
    }
  }
  __syncthreads();   // the ring is idle: this wave's rows of O leave through WR x 256 bytes of it
  if (!wave_live) return;
  bf16_t* img = smem + wave * WR * kD;
#pragma unroll
  for (int c = 0; c < CH; ++c) {
    const float lt = row4_sum(st[c].l);
    if ((lane >> 4) == 0 && ok[c])
      a.lse[((long)b * a.T + trow[c]) * a.H + h0 + grow[c]] = lt > 0.f ? st[c].m + __log2f(lt) : INFINITY;
    stage_rows(img, 16 * c, st[c].o, lt > 0.f ? 1.f / lt : 0.f, lane);
  }
  flush_rows<WR>(img, a.o + (long)b * a.ob, a, r0w, R, h0, lane);
}

// the launch of ljs_attn_chunk128 over a cache of the template's kind (c.kind has chosen it)
template <bool MX8>
int chunk128_launch(const void* q, const LjsCache& c, void* o, void* lse, const void* lens, int B, int T, int H,
                    const long* sq, const long* so, float scale, hipStream_t st) {
  constexpr long ES = MX8 ? 1 : 2;       // bytes per cache element
  const int Hkv = c.Hkv, cap = c.cap;
  if (B < 1 || T < 1 || H < 1 || Hkv < 1 || cap < 1 || H % Hkv != 0 || H / Hkv > kMaxG || !(scale > 0.f) ||
      B > 65535 || Hkv > 65535 || (long)T * H > 0x3fffffffL || (long)B * T * H > 0x7fffffffL || !lens || !lse ||
      (((uintptr_t)lens) & 3u) || (((uintptr_t)lse) & 3u))
    return (int)hipErrorInvalidValue;
  if (!bf16_aligned(q, sq) || !bf16_aligned(o, so) || !cache_aligned(c)) return (int)hipErrorInvalidValue;
  // a load reaches up to one tile past the cache
  if (!cache_reach_ok(c, (long)cap + kKeys)) return (int)hipErrorInvalidValue;
  Chunk128Args a{};
  a.q = (const bf16_t*)q;
  a.kc = (const unsigned char*)c.k;
  a.vc = (const unsigned char*)c.v;
  a.o = (bf16_t*)o;
  a.lse = (float*)lse;
  a.lens = (const int*)lens;
  a.qb = sq[0]; a.qt = sq[1]; a.qh = sq[2];
  a.ob = so[0]; a.ot = so[1]; a.oh = so[2];
  a.kb = c.sk[0] * ES; a.ks = c.sk[1] * ES; a.kh = c.sk[2] * ES;
  a.vb = c.sv[0] * ES; a.vs = c.sv[1] * ES; a.vh = c.sv[2] * ES;
  if (MX8) {
    a.ksc = (const unsigned char*)c.ks;
    a.vsc = (const unsigned char*)c.vs;
    a.ksb = c.sks[0]; a.kss = c.sks[1]; a.ksh = c.sks[2];
    a.vsb = c.svs[0]; a.vss = c.svs[1]; a.vsh = c.svs[2];
  }
  a.T = T; a.H = H; a.G = H / Hkv; a.cap = cap;
  a.scale_log2 = scale * kLog2e;
  int plan[4];
  if (ljs_chunk_plan(B, T, H, Hkv, ljs_device_cus(), plan) != 0) return (int)hipErrorInvalidValue;
  int rows = plan[0];
  unsigned gx = (unsigned)plan[1];
  if (const int forced = ljs_chunk_get_rows()) {
    rows = forced;
    gx = (unsigned)(((long)T * a.G + rows - 1) / rows);
  }
  const dim3 grid(gx, (unsigned)Hkv, (unsigned)B);
  if (rows == 128) hipLaunchKernelGGL((attn_chunk128_kernel<128, MX8>), grid, dim3(kThreads), 0, st, a);
  else hipLaunchKernelGGL((attn_chunk128_kernel<64, MX8>), grid, dim3(kThreads), 0, st, a);
  ljs_launch_rec(rows == 128 ? (MX8 ? "attn_chunk128<R128,mx8>" : "attn_chunk128<R128>")
                             : (MX8 ? "attn_chunk128<R64,mx8>" : "attn_chunk128<R64>"), grid, kThreads);
  return (int)hipGetLastError();
}

}  // namespace

// ljs_attn_chunk (prefill.hip) at head dim 128: q (B, T, H, 128) over the cache c (cache_common.h; either kind, dim
// 128) -> o (B, T, H, 128) bf16, lse (B, T, H) f32.  The same arguments, the same refusals (hipErrorInvalidValue with
// nothing launched or recorded), and a cache whose head dim is not 128 is refused too.  One launch.
LJS_API int ljs_attn_chunk128(const void* q, const LjsCache* c, void* o, void* lse, const void* lens, int B, int T,
                              int H, const long* sq, const long* so, float scale, hipStream_t st) {
  if (!c || c->dim != kD) return (int)hipErrorInvalidValue;
  return c->kind == kCacheMx8 ? chunk128_launch<true>(q, *c, o, lse, lens, B, T, H, sq, so, scale, st)
                              : chunk128_launch<false>(q, *c, o, lse, lens, B, T, H, sq, so, scale, st);
}
