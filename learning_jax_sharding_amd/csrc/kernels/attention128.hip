// LJS_HIPCC_FLAGS: -Xclang -target-feature -Xclang -packed-fp32-ops
// Flash attention for head_dim 128 on gfx950, forward and backward (attention.hip is the head_dim 64
// file; semantics, conventions and rounding points are exactly its own: bf16 (B, S, H, 128) operands
// with arbitrary batch / seq / head strides, k / v of Hkv = H / G heads, causal with q_offset, lse =
// log2 of the scaled-score partition function with +inf / o = 0 for a row that sees no key, P and dS
// rounded to bf16 before their second products, delta the f32 row sum of bf16 dO times the stored O,
// the dP accumulators seeded with -delta, one rounding of every output).
//
// The layout trick is attention.hip's: S^T = K . Q^T with the 16x16x32 bf16 MFMA, so a lane owns one
// query (the accumulator column) and the row softmax stays in-lane; P^T leaves the accumulators as
// the B operand of O^T = V^T . P^T, V^T coming from the transposing LDS read.  What is new at 128:
//
//   * LDS image [64 rows][128 d] bf16 with 256-byte rows of 16 chunks of 16 bytes, chunk c of row r at
//     c ^ swz(r).  swz's bits (3..0) are (r2 ^ r3, r1, r0, r2) of the row number: 16 consecutive rows
//     of one chunk (a ds_read_b128 operand column) land on 16 different chunk positions, 8 of them on
//     8 different positions mod 8, and the 8 rows x 32 bytes of a ds_read_b64_tr_b16 half-wave on 8
//     different 32-byte pairs (4 consecutive rows on 4 different pairs mod 4): no two lanes of one
//     issue group share a bank in either pattern, with 64 banks or with 32.  img16 (128-byte rows)
//     does not carry over.  Tiles arrive by LDS-DMA with the swizzle on the source address.
//   * forward: 4 waves x 32 queries (two 16-query MFMA chains that share every K and V fragment), Q
//     fragments in registers (4 k-steps), 64-key K and V tiles through a two-stage ring: 64 KiB per
//     block, two blocks per CU, one barrier per key tile.
//   * backward: ONE launch of two block roles.  dQ blocks take 128 queries of one head and sweep the
//     visible key tiles through the same ring.  dK/dV blocks take one 64-key tile of one K/V head (16
//     keys per wave: dK and dV are 64 f32 accumulator registers per lane) and sweep the visible query
//     tiles of all G query heads of the group in a fixed order (head, then query tile), accumulating
//     in f32 and writing dK / dV once: no per-query-head scratch, no reduce pass, no atomics.  Each
//     role forms delta itself (the dQ blocks from their register fragments, the dK/dV blocks from
//     the rows of O and dO they load beside the tile DMA), so there is no delta buffer and no order
//     between the roles.
//   * every output row tile leaves through the idle ring as whole 256-byte rows.
#include "common.h"

#include <cstdio>

namespace {

constexpr int D = 128;     // head dim
constexpr int BLK = 64;    // keys (forward, dQ) / queries (dK/dV) per tile
constexpr int QB = 128;    // queries per forward / dQ block
constexpr int TILE = BLK * D;   // elements of one LDS image (16 KiB)
constexpr float LOG2E = 1.4426950408889634f;

struct Attn128Args {
  const bf16_t* q; const bf16_t* k; const bf16_t* v; const bf16_t* o; const bf16_t* dout;
  bf16_t* out;                   // forward: O (with the o strides)
  bf16_t* dq; bf16_t* dk; bf16_t* dv;
  float* lse;                    // [B][H][Sq], log2 domain of the scaled scores
  long q_sb, q_ss, q_sh, k_sb, k_ss, k_sh, v_sb, v_ss, v_sh, o_sb, o_ss, o_sh, do_sb, do_ss, do_sh;
  long dq_sb, dq_ss, dq_sh, dk_sb, dk_ss, dk_sh, dv_sb, dv_ss, dv_sh;
  int B, Sq, Sk, H, Hkv, G;      // G = H / Hkv: query head h reads K/V head h / G
  int nqb, nkt;                  // 128-query blocks and 64-key tiles per head
  float scale, scale_log2;
  int causal, q_offset;
};

__device__ __forceinline__ float fast_exp2(float x) { return __builtin_amdgcn_exp2f(x); }

// ---- LDS image (see the header): element index of 16-byte chunk c16 / 8-byte piece c8 of a row
__device__ __forceinline__ int swz(int row) {
  return ((row & 3) << 1) | ((row >> 2) & 1) | ((((row >> 2) ^ (row >> 3)) & 1) << 3);
}
__device__ __forceinline__ int img16(int row, int c16) { return row * D + ((c16 ^ swz(row)) << 3); }
__device__ __forceinline__ int img8(int row, int c8) { return img16(row, c8 >> 1) + ((c8 & 1) << 2); }

// The lane parts of the fragment addresses, worked out once per kernel and shared by the masked and
// the unmasked tile bodies: the swizzle reads the row number's low four bits only, so a row base
// that is a multiple of 16 is a plain (immediate) offset on top of them.
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
// MFMA operand from rows [rb, rb + 16) of an image (rb % 16 == 0), k-step ks (d 32 ks .. 32 ks + 31)
__device__ __forceinline__ bf16x8 frag_rows(const bf16_t* lds, int rb, int ks, const LaneOff& f) {
  return __builtin_bit_cast(bf16x8, *reinterpret_cast<const u32x4*>(lds + rb * D + f.rows[ks]));
}
// MFMA A operand A[m = d][k = row]: d = 16 dt + (lane & 15); elements 0..3 = rows R0 + 4 g + 0..3,
// elements 4..7 = rows R0 + 16 + 4 g + 0..3 (R0 % 16 == 0, g the lane's 16-lane group)
__device__ __forceinline__ bf16x8 frag_tr(const bf16_t* lds, int R0, int dt, const LaneOff& f) {
  return join_bf16x8(lds_read_tr16(lds + R0 * D + f.tr[dt]), lds_read_tr16(lds + (R0 + 16) * D + f.tr[dt]));
}
// a lane's 16-byte row fragment (8 consecutive d) straight from global memory
__device__ __forceinline__ bf16x8 load_row_frag(const bf16_t* __restrict__ rowp, bool ok, int ks, int lane) {
  if (!ok) return __builtin_bit_cast(bf16x8, u32x4{0, 0, 0, 0});
  return __builtin_bit_cast(bf16x8, *reinterpret_cast<const u32x4*>(rowp + 32 * ks + 8 * (lane >> 4)));
}
__device__ __forceinline__ float dot_bf16x8(const u32x4& x, const u32x4& y, float acc) {
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    acc = fmaf(__uint_as_float(x[k] << 16), __uint_as_float(y[k] << 16), acc);
    acc = fmaf(__uint_as_float(x[k] & 0xffff0000u), __uint_as_float(y[k] & 0xffff0000u), acc);
  }
  return acc;
}

// Rows r0 .. r0 + 63 of a (seq, d) slab (`rows` rows, row stride ld elements) into the image `lds` by
// LDS-DMA: 16 pieces of 4 rows x 256 bytes, four per wave; rows past the end read as zeros.  The
// resource is rebased on the tile, so the 32-bit offsets only span 64 rows (the plan bounds ld).
__device__ __forceinline__ void dma_tile(const bf16_t* base, long ld, int r0, int rows, bf16_t* lds, int wave,
                                         int lane) {
  const int nr = rows - r0 < BLK ? rows - r0 : BLK;
  const u32x4 rs = rsrc_u4(base + (long)r0 * ld, 2 * ((long)(nr - 1) * ld + D));
  const int ld32 = (int)ld;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int pc = wave + 4 * i, row = 4 * pc + (lane >> 4);
    const int c = ((lane & 15) ^ swz(row)) * 8;
    dma_lds_x4(rs, row < nr ? (row * ld32 + c) * 2 : 0x7ffffff0, lds + pc * 512);
  }
}

// A lane's 32 d-values (8 tiles of 4) of local row rbase + (lane & 15) into a wave-private [rows][128]
// bf16 image (the same chunk swizzle), and NR staged rows out as whole 256-byte rows: 4 rows per
// 16-byte-per-lane store instead of 8-byte pieces of 16 rows each.
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
__device__ __forceinline__ void flush_rows(const bf16_t* img, bf16_t* base, long ld, int row0, int rlim, int lane) {
  u32x4 v[NR / 4];
#pragma unroll
  for (int i = 0; i < NR / 4; ++i) v[i] = *reinterpret_cast<const u32x4*>(img + img16(4 * i + (lane >> 4), lane & 15));
#pragma unroll
  for (int i = 0; i < NR / 4; ++i) {
    const int r = row0 + 4 * i + (lane >> 4);
    if (r < rlim) *reinterpret_cast<u32x4*>(base + (long)r * ld + 8 * (lane & 15)) = v[i];
  }
}

// the DMA is issued from asm (common.h): wait for this wave's pieces, then for everyone's
__device__ __forceinline__ void tiles_landed() {
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();
}

// block id -> (query block, head, batch) of the forward and the dQ role: the G query heads of a K/V
// group are adjacent (their K / V tiles meet in L2), and under causal the longest blocks come first
struct QItem {
  int qb, h, hk, b;
};
__device__ __forceinline__ QItem q_item(const Attn128Args& a, int t) {
  QItem it;
  const int gi = t % a.G;
  t /= a.G;
  const int qbi = t % a.nqb;
  t /= a.nqb;
  it.hk = t % a.Hkv;
  it.b = t / a.Hkv;
  it.qb = a.causal ? a.nqb - 1 - qbi : qbi;
  it.h = it.hk * a.G + gi;
  return it;
}
// key tiles a 128-query block sees
__device__ __forceinline__ int visible_key_tiles(const Attn128Args& a, int qb) {
  int kend = a.Sk;
  if (a.causal) kend = min(a.Sk, a.q_offset + (qb + 1) * QB);
  return kend > 0 ? (kend + BLK - 1) / BLK : 0;
}

// ============================================================================ forward
struct FwdState {
  f32x4 o[8];
  float m, l;
};

// one 64-key tile for a wave's two 16-query chains (rows qrow0 + 16 t + (lane & 15))
template <bool MASK>
__device__ __forceinline__ void fwd_tile(const Attn128Args& a, FwdState (&st)[2], const bf16_t* Kt, const bf16_t* Vt,
                                         const bf16x8 (&qf)[2][4], int kbase, int qrow0, int lane, const LaneOff& f) {
  const int g = lane >> 4;
  f32x4 s[2][4];
#pragma unroll
  for (int jt = 0; jt < 4; ++jt) {
#pragma unroll
    for (int t = 0; t < 2; ++t) s[t][jt] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int ks = 0; ks < 4; ++ks) {
      const bf16x8 kf = frag_rows(Kt, 16 * jt, ks, f);
#pragma unroll
      for (int t = 0; t < 2; ++t) s[t][jt] = mfma16x16x32(kf, qf[t][ks], s[t][jt]);
    }
  }
  u32x4 pb[2][2];
#pragma unroll
  for (int t = 0; t < 2; ++t) {
    if constexpr (MASK) {
      const int qlim = qrow0 + 16 * t + (lane & 15) + a.q_offset;
#pragma unroll
      for (int jt = 0; jt < 4; ++jt)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int key = kbase + 16 * jt + 4 * g + r;
          const bool masked = key >= a.Sk || (a.causal && key > qlim);
          s[t][jt][r] = masked ? -INFINITY : s[t][jt][r];
        }
    }
    float tmax = fmaxf(fmaxf(s[t][0][0], s[t][0][1]), fmaxf(s[t][0][2], s[t][0][3]));
#pragma unroll
    for (int jt = 1; jt < 4; ++jt)
      tmax = fmaxf(tmax, fmaxf(fmaxf(s[t][jt][0], s[t][jt][1]), fmaxf(s[t][jt][2], s[t][jt][3])));
    tmax = row4_max(tmax);
    // scores are compared raw (scale > 0 keeps the order); the scale is one FMA in front of v_exp_f32
    const float m_new = fmaxf(st[t].m, tmax * a.scale_log2);
    float m_use = m_new;
    if constexpr (MASK) m_use = m_new == -INFINITY ? 0.f : m_new;   // no key seen so far: p = 0
    const float alpha = fast_exp2(st[t].m - m_use);
    float ps0 = 0.f, ps1 = 0.f;
#pragma unroll
    for (int jt = 0; jt < 4; ++jt)
#pragma unroll
      for (int r = 0; r < 4; r += 2) {
        const float p0 = fast_exp2(fmaf(s[t][jt][r], a.scale_log2, -m_use));
        const float p1 = fast_exp2(fmaf(s[t][jt][r + 1], a.scale_log2, -m_use));
        s[t][jt][r] = p0;
        s[t][jt][r + 1] = p1;
        ps0 += p0;
        ps1 += p1;
      }
    // no lane's running max moved (the usual case after the first key tiles): alpha is exactly 1,
    // or the row has seen no key and O is 0, so the O rescale is skipped wave-uniformly
    const bool rescale = !__all(m_new == st[t].m);
    st[t].l = st[t].l * alpha + (ps0 + ps1);
    st[t].m = m_new;
    if (rescale) {
#pragma unroll
      for (int dt = 0; dt < 8; ++dt) st[t].o[dt] = st[t].o[dt] * alpha;
    }
#pragma unroll
    for (int s2 = 0; s2 < 2; ++s2) {
      pb[t][s2][0] = pack_bf16x2(s[t][2 * s2][0], s[t][2 * s2][1]);
      pb[t][s2][1] = pack_bf16x2(s[t][2 * s2][2], s[t][2 * s2][3]);
      pb[t][s2][2] = pack_bf16x2(s[t][2 * s2 + 1][0], s[t][2 * s2 + 1][1]);
      pb[t][s2][3] = pack_bf16x2(s[t][2 * s2 + 1][2], s[t][2 * s2 + 1][3]);
    }
  }
#pragma unroll
  for (int s2 = 0; s2 < 2; ++s2)
#pragma unroll
    for (int dt = 0; dt < 8; ++dt) {
      const bf16x8 va = frag_tr(Vt, 32 * s2, dt, f);
#pragma unroll
      for (int t = 0; t < 2; ++t) st[t].o[dt] = mfma16x16x32(va, __builtin_bit_cast(bf16x8, pb[t][s2]), st[t].o[dt]);
    }
}

// MASK = false: no tile can need masking (not causal, Sk a multiple of 64), and the masked tile body
// is not compiled in; MASK = true decides per tile and wave.
template <bool MASK>
__global__ __launch_bounds__(256, 2) void attn128_fwd_kernel(Attn128Args a) {
  __shared__ __attribute__((aligned(16))) bf16_t smem[4 * TILE];   // [stage][K | V]
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const LaneOff f = lane_off(lane);
  const QItem it = q_item(a, xcd_remap(blockIdx.x, gridDim.x));
  const int b = it.b, h = it.h;
  const bf16_t* kb = a.k + b * a.k_sb + it.hk * a.k_sh;
  const bf16_t* vb = a.v + b * a.v_sb + it.hk * a.v_sh;
  const int nkt = visible_key_tiles(a, it.qb);
  const int qrow0 = it.qb * QB + 32 * wave;

  bf16x8 qf[2][4];
#pragma unroll
  for (int t = 0; t < 2; ++t) {
    const int qrow = qrow0 + 16 * t + (lane & 15);
    const bf16_t* qp = a.q + b * a.q_sb + (long)qrow * a.q_ss + h * a.q_sh;
#pragma unroll
    for (int ks = 0; ks < 4; ++ks) qf[t][ks] = load_row_frag(qp, qrow < a.Sq, ks, lane);
  }
  auto issue = [&](int kt) {
    bf16_t* st = smem + (kt & 1) * 2 * TILE;
    dma_tile(kb, a.k_ss, kt * BLK, a.Sk, st, wave, lane);
    dma_tile(vb, a.v_ss, kt * BLK, a.Sk, st + TILE, wave, lane);
  };
  FwdState st[2];
#pragma unroll
  for (int t = 0; t < 2; ++t) {
#pragma unroll
    for (int i = 0; i < 8; ++i) st[t].o[i] = f32x4{0.f, 0.f, 0.f, 0.f};
    st[t].m = -INFINITY;
    st[t].l = 0.f;
  }
  if (nkt > 0) issue(0);
#pragma unroll 1
  for (int kt = 0; kt < nkt; ++kt) {
    tiles_landed();   // tile kt is in its stage, and every wave is done with tile kt - 1
    if (kt + 1 < nkt) issue(kt + 1);
    const bf16_t* Kt = smem + (kt & 1) * 2 * TILE;
    const int kbase = kt * BLK;
    if constexpr (MASK) {
      if (a.causal && kbase > qrow0 + 31 + a.q_offset) continue;   // wholly above this wave's diagonal
      const bool need_mask = kbase + BLK > a.Sk || (a.causal && kbase + BLK - 1 > qrow0 + a.q_offset);
      if (need_mask) fwd_tile<true>(a, st, Kt, Kt + TILE, qf, kbase, qrow0, lane, f);
      else fwd_tile<false>(a, st, Kt, Kt + TILE, qf, kbase, qrow0, lane, f);
    } else {
      fwd_tile<false>(a, st, Kt, Kt + TILE, qf, kbase, qrow0, lane, f);
    }
  }
  __syncthreads();   // the ring is idle: this wave's 32 rows of O leave through 8 KiB of it
  bf16_t* img = smem + wave * 32 * D;
#pragma unroll
  for (int t = 0; t < 2; ++t) {
    const float lt = row4_sum(st[t].l);
    const int qrow = qrow0 + 16 * t + (lane & 15);
    if ((lane >> 4) == 0 && qrow < a.Sq)
      a.lse[((long)b * a.H + h) * a.Sq + qrow] = lt > 0.f ? st[t].m + __log2f(lt) : INFINITY;
    stage_rows(img, 16 * t, st[t].o, lt > 0.f ? 1.f / lt : 0.f, lane);
  }
  flush_rows<32>(img, a.out + b * a.o_sb + h * a.o_sh, a.o_ss, qrow0, a.Sq, lane);
}

// ============================================================================ backward: dQ role
template <bool MASK>
__device__ __forceinline__ void dq_tile(const Attn128Args& a, const bf16_t* Kt, const bf16_t* Vt,
                                        const bf16x8 (&qf)[2][4], const bf16x8 (&df)[2][4], const float (&lse_q)[2],
                                        const float (&ndl_q)[2], f32x4 (&dq)[2][8], int kbase, int qrow0, bool need_mask,
                                        int lane, const LaneOff& f) {
  const int g = lane >> 4;
#pragma unroll
  for (int s2 = 0; s2 < 2; ++s2) {
    u32x4 sbu[2];   // [chain]: dS of keys 32 s2 .. + 31 as bf16, in the accumulator k-order (half a tile at a
                    // time: the whole tile's dS held 8 more registers and spilled beside the dK/dV role)
#pragma unroll
    for (int jt = 2 * s2; jt < 2 * s2 + 2; ++jt) {
      f32x4 s[2], dp[2];
#pragma unroll
      for (int i = 0; i < 2; ++i) {
        s[i] = f32x4{0.f, 0.f, 0.f, 0.f};
        dp[i] = f32x4{ndl_q[i], ndl_q[i], ndl_q[i], ndl_q[i]};
      }
#pragma unroll
      for (int ks = 0; ks < 4; ++ks) {
        const bf16x8 kf = frag_rows(Kt, 16 * jt, ks, f), vf = frag_rows(Vt, 16 * jt, ks, f);
#pragma unroll
        for (int i = 0; i < 2; ++i) {
          s[i] = mfma16x16x32(kf, qf[i][ks], s[i]);
          dp[i] = mfma16x16x32(vf, df[i][ks], dp[i]);
        }
      }
#pragma unroll
      for (int i = 0; i < 2; ++i) {
        float p[4], ds[4];
#pragma unroll
        for (int r = 0; r < 4; ++r) p[r] = fast_exp2(fmaf(s[i][r], a.scale_log2, -lse_q[i]));
        if constexpr (MASK) {
          if (need_mask) {
#pragma unroll
            for (int r = 0; r < 4; ++r) {
              const int key = kbase + 16 * jt + 4 * g + r;
              const bool ok = key < a.Sk && !(a.causal && key > qrow0 + 16 * i + (lane & 15) + a.q_offset);
              p[r] = ok ? p[r] : 0.f;
            }
          }
        }
#pragma unroll
        for (int r = 0; r < 4; ++r) ds[r] = p[r] * dp[i][r];
        sbu[i][2 * (jt & 1)] = pack_bf16x2(ds[0], ds[1]);
        sbu[i][2 * (jt & 1) + 1] = pack_bf16x2(ds[2], ds[3]);
      }
    }
    // dQ^T += K^T dS^T   (k = keys)
#pragma unroll
    for (int dt = 0; dt < 8; ++dt) {
      const bf16x8 ka = frag_tr(Kt, 32 * s2, dt, f);
#pragma unroll
      for (int i = 0; i < 2; ++i) dq[i][dt] = mfma16x16x32(ka, __builtin_bit_cast(bf16x8, sbu[i]), dq[i][dt]);
    }
  }
}

template <bool MASK>
__device__ __forceinline__ void dq_body(const Attn128Args& a, const QItem& it, bf16_t* smem) {
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const LaneOff f = lane_off(lane);
  const int b = it.b, h = it.h;
  const int qrow0 = it.qb * QB + 32 * wave;
  bf16x8 qf[2][4], df[2][4];
  float lse_q[2], ndl_q[2];
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    const int qrow = qrow0 + 16 * i + (lane & 15);
    const bool qok = qrow < a.Sq;
    const bf16_t* qp = a.q + b * a.q_sb + (long)qrow * a.q_ss + h * a.q_sh;
    const bf16_t* dop = a.dout + b * a.do_sb + (long)qrow * a.do_ss + h * a.do_sh;
    const bf16_t* op = a.o + b * a.o_sb + (long)qrow * a.o_ss + h * a.o_sh;
    float sacc = 0.f;
#pragma unroll
    for (int ks = 0; ks < 4; ++ks) {
      qf[i][ks] = load_row_frag(qp, qok, ks, lane);
      df[i][ks] = load_row_frag(dop, qok, ks, lane);
      sacc = dot_bf16x8(__builtin_bit_cast(u32x4, load_row_frag(op, qok, ks, lane)),
                        __builtin_bit_cast(u32x4, df[i][ks]), sacc);
    }
    lse_q[i] = qok ? a.lse[((long)b * a.H + h) * a.Sq + qrow] : INFINITY;   // +inf: P = 0
    ndl_q[i] = -row4_sum(sacc);   // delta, kept negated: it seeds the dP accumulators
  }
  const bf16_t* kb = a.k + b * a.k_sb + it.hk * a.k_sh;
  const bf16_t* vb = a.v + b * a.v_sb + it.hk * a.v_sh;
  const int nkt = visible_key_tiles(a, it.qb);
  auto issue = [&](int kt) {
    bf16_t* st = smem + (kt & 1) * 2 * TILE;
    dma_tile(kb, a.k_ss, kt * BLK, a.Sk, st, wave, lane);
    dma_tile(vb, a.v_ss, kt * BLK, a.Sk, st + TILE, wave, lane);
  };
  f32x4 dq[2][8];
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 8; ++j) dq[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
  if (nkt > 0) issue(0);
#pragma unroll 1
  for (int kt = 0; kt < nkt; ++kt) {
    tiles_landed();
    if (kt + 1 < nkt) issue(kt + 1);
    const bf16_t* Kt = smem + (kt & 1) * 2 * TILE;
    const int kbase = kt * BLK;
    if constexpr (MASK) {
      if (a.causal && kbase > qrow0 + 31 + a.q_offset) continue;
      const bool need_mask = kbase + BLK > a.Sk || (a.causal && kbase + BLK - 1 > qrow0 + a.q_offset);
      dq_tile<true>(a, Kt, Kt + TILE, qf, df, lse_q, ndl_q, dq, kbase, qrow0, need_mask, lane, f);
    } else {
      dq_tile<false>(a, Kt, Kt + TILE, qf, df, lse_q, ndl_q, dq, kbase, qrow0, false, lane, f);
    }
  }
  __syncthreads();
  bf16_t* img = smem + wave * 32 * D;
#pragma unroll
  for (int i = 0; i < 2; ++i) stage_rows(img, 16 * i, dq[i], a.scale, lane);
  flush_rows<32>(img, a.dq + b * a.dq_sb + h * a.dq_sh, a.dq_ss, qrow0, a.Sq, lane);
}

// ============================================================================ backward: dK/dV role
// one 64-query tile (Q and dO images, rc = [lse | -delta] of its rows) for a wave's 16 keys
template <bool MASK>
__device__ __forceinline__ void dkv_tile(const Attn128Args& a, const bf16_t* Qt, const bf16_t* Dt, const float* rc,
                                         const bf16x8 (&kr)[4], const bf16x8 (&vr)[4], f32x4 (&dk)[8], f32x4 (&dv)[8],
                                         int q0, int key, bool need_mask, int lane, const LaneOff& f) {
  const int g = lane >> 4;
#pragma unroll
  for (int s2 = 0; s2 < 2; ++s2) {
    u32x4 pbu, sbu;
#pragma unroll
    for (int tt = 0; tt < 2; ++tt) {
      const int t = 2 * s2 + tt;
      const f32x4 lse = *reinterpret_cast<const f32x4*>(rc + 16 * t + 4 * g);
      f32x4 s = f32x4{0.f, 0.f, 0.f, 0.f}, dp = *reinterpret_cast<const f32x4*>(rc + BLK + 16 * t + 4 * g);
#pragma unroll
      for (int ks = 0; ks < 4; ++ks) {
        s = mfma16x16x32(frag_rows(Qt, 16 * t, ks, f), kr[ks], s);
        dp = mfma16x16x32(frag_rows(Dt, 16 * t, ks, f), vr[ks], dp);
      }
      float p[4], ds[4];
#pragma unroll
      for (int r = 0; r < 4; ++r) p[r] = fast_exp2(fmaf(s[r], a.scale_log2, -lse[r]));
      if constexpr (MASK) {
        if (need_mask) {
#pragma unroll
          for (int r = 0; r < 4; ++r) p[r] = key > q0 + 16 * t + 4 * g + r + a.q_offset ? 0.f : p[r];
        }
      }
#pragma unroll
      for (int r = 0; r < 4; ++r) ds[r] = p[r] * dp[r];
      pbu[2 * tt] = pack_bf16x2(p[0], p[1]);
      pbu[2 * tt + 1] = pack_bf16x2(p[2], p[3]);
      sbu[2 * tt] = pack_bf16x2(ds[0], ds[1]);
      sbu[2 * tt + 1] = pack_bf16x2(ds[2], ds[3]);
    }
    // dV^T += dO^T P ; dK^T += Q^T dS   (k = the 32 queries of this half)
#pragma unroll
    for (int dt = 0; dt < 8; ++dt) {
      const bf16x8 oa = frag_tr(Dt, 32 * s2, dt, f);
      const bf16x8 qa = frag_tr(Qt, 32 * s2, dt, f);
      dv[dt] = mfma16x16x32(oa, __builtin_bit_cast(bf16x8, pbu), dv[dt]);
      dk[dt] = mfma16x16x32(qa, __builtin_bit_cast(bf16x8, sbu), dk[dt]);
    }
  }
}

// dK, dV of key tile kt of K/V head hk: the sweep runs over (query head of the group, query tile) in
// that order.  Q and dO tiles arrive by LDS-DMA into a two-stage ring; beside them each thread loads a
// quarter row of O and dO (and the row's lse) of the same tile into registers and, after the
// current tile's math, leaves the row's lse and -delta in rc for the next one.  Rows past Sq get
// lse = +inf (P = 0) and zero operands; keys past Sk are computed on zeros and never stored.
template <bool MASK>
__device__ __forceinline__ void dkv_body(const Attn128Args& a, int kt, int hk, int b, bf16_t* smem, float* rc) {
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const LaneOff f = lane_off(lane);
  const int key0 = kt * BLK + 16 * wave, key = key0 + (lane & 15);
  bf16x8 kr[4], vr[4];
  {
    const bf16_t* kp = a.k + b * a.k_sb + (long)key * a.k_ss + hk * a.k_sh;
    const bf16_t* vp = a.v + b * a.v_sb + (long)key * a.v_ss + hk * a.v_sh;
#pragma unroll
    for (int ks = 0; ks < 4; ++ks) {
      kr[ks] = load_row_frag(kp, key < a.Sk, ks, lane);
      vr[ks] = load_row_frag(vp, key < a.Sk, ks, lane);
    }
  }
  int qstart = 0;   // the first query tile that sees the tile's first key
  if (MASK && a.causal) qstart = max(0, kt * BLK - a.q_offset) / BLK * BLK;
  const int nqt = qstart < a.Sq ? (a.Sq - qstart + BLK - 1) / BLK : 0;
  const int total = nqt * a.G;
  const bool active = key0 < a.Sk;
  const int row = tid >> 2, c = tid & 3;   // delta: 4 threads per query row, 32 d each

  u32x4 po[4], pd[4];
  float pl;
  auto prefetch = [&](int n) {
    const int gi = n / nqt, q0 = qstart + (n - gi * nqt) * BLK, h = hk * a.G + gi;
    bf16_t* st = smem + (n & 1) * 2 * TILE;
    dma_tile(a.q + b * a.q_sb + h * a.q_sh, a.q_ss, q0, a.Sq, st, wave, lane);
    dma_tile(a.dout + b * a.do_sb + h * a.do_sh, a.do_ss, q0, a.Sq, st + TILE, wave, lane);
    const int r = q0 + row;
    const bool ok = r < a.Sq;
    const bf16_t* op = a.o + b * a.o_sb + (long)r * a.o_ss + h * a.o_sh + 32 * c;
    const bf16_t* dp = a.dout + b * a.do_sb + (long)r * a.do_ss + h * a.do_sh + 32 * c;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      po[i] = ok ? *reinterpret_cast<const u32x4*>(op + 8 * i) : u32x4{0, 0, 0, 0};
      pd[i] = ok ? *reinterpret_cast<const u32x4*>(dp + 8 * i) : u32x4{0, 0, 0, 0};
    }
    pl = ok ? a.lse[((long)b * a.H + h) * a.Sq + r] : INFINITY;
  };
  auto finish = [&](int n) {
    float sacc = 0.f;
#pragma unroll
    for (int i = 0; i < 4; ++i) sacc = dot_bf16x8(po[i], pd[i], sacc);
    sacc += __shfl_xor(sacc, 1, 64);
    sacc += __shfl_xor(sacc, 2, 64);
    if (c == 0) {
      rc[(n & 1) * 2 * BLK + row] = pl;
      rc[(n & 1) * 2 * BLK + BLK + row] = -sacc;
    }
  };
  f32x4 dk[8], dv[8];
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    dk[i] = f32x4{0.f, 0.f, 0.f, 0.f};
    dv[i] = f32x4{0.f, 0.f, 0.f, 0.f};
  }
  if (total > 0) {
    prefetch(0);
    finish(0);
  }
#pragma unroll 1
  for (int n = 0; n < total; ++n) {
    tiles_landed();   // tile n (images and rc) is in its stage, and every wave is done with tile n - 1
    const bool more = n + 1 < total;
    if (more) prefetch(n + 1);
    const bf16_t* Qt = smem + (n & 1) * 2 * TILE;
    const float* rcn = rc + (n & 1) * 2 * BLK;
    const int q0 = qstart + (n % nqt) * BLK;
    if (active) {
      if constexpr (MASK) {
        // causal: nothing of the tile sees this wave's keys / every query sees all of them
        const bool none = a.causal && key0 > q0 + BLK - 1 + a.q_offset;
        const bool need_mask = a.causal && key0 + 15 > q0 + a.q_offset;
        if (!none) dkv_tile<true>(a, Qt, Qt + TILE, rcn, kr, vr, dk, dv, q0, key, need_mask, lane, f);
      } else {
        dkv_tile<false>(a, Qt, Qt + TILE, rcn, kr, vr, dk, dv, q0, key, false, lane, f);
      }
    }
    if (more) finish(n + 1);
  }
  __syncthreads();   // the ring is idle: this wave's 16 rows of dK and of dV leave through 8 KiB of it
  if (!active) return;
  bf16_t* ik = smem + wave * 32 * D;
  bf16_t* iv = ik + 16 * D;
  stage_rows(ik, 0, dk, a.scale, lane);
  stage_rows(iv, 0, dv, 1.f, lane);
  flush_rows<16>(ik, a.dk + b * a.dk_sb + hk * a.dk_sh, a.dk_ss, key0, a.Sk, lane);
  flush_rows<16>(iv, a.dv + b * a.dv_sb + hk * a.dv_sh, a.dv_ss, key0, a.Sk, lane);
}

// Both roles in one grid: [dK/dV blocks | dQ blocks].  The dK/dV blocks come first: each sweeps G
// heads, and under causal the early key tiles see the most queries, so the longest blocks start first.
// MASK = false: not causal (key and query tails need no mask in the dK/dV role) and Sk % 64 == 0.
template <bool MASK>
__global__ __launch_bounds__(256, 2) void attn128_bwd_kernel(Attn128Args a) {
  __shared__ __attribute__((aligned(16))) bf16_t smem[4 * TILE];   // ring: [stage][K | V] or [stage][Q | dO]
  __shared__ __attribute__((aligned(16))) float rc[2 * 2 * BLK];   // dK/dV role: [stage][lse | -delta]
  const int t = xcd_remap(blockIdx.x, gridDim.x);
  const int ndkv = a.nkt * a.Hkv * a.B;
  if (t < ndkv) {
    const int u = t / a.nkt;
    dkv_body<MASK>(a, t - u * a.nkt, u % a.Hkv, u / a.Hkv, smem, rc);
  } else {
    dq_body<MASK>(a, q_item(a, t - ndkv), smem);
  }
}

// ---------------------------------------------------------------------------- plan and entry points
#define LJS_ATTN128_INSTANCES(X)        \
  X(kFwd0, "attn128_fwd<mask=0>")       \
  X(kFwd1, "attn128_fwd<mask=1>")       \
  X(kBwd0, "attn128_bwd<mask=0>")       \
  X(kBwd1, "attn128_bwd<mask=1>")
#define X(id, name) id,
enum Inst128 { LJS_ATTN128_INSTANCES(X) kInstCount };
#undef X
#define X(id, name) name,
const char* const kInstName[kInstCount] = {LJS_ATTN128_INSTANCES(X)};
#undef X

struct Plan128 {
  hipError_t err;
  Inst128 inst;
  unsigned grid, block;
};

// an operand on the 16-byte grid: base and (batch, seq, head) strides; rows that the LDS-DMA or a
// 32-bit row offset walks need a sequence stride in [0, 2^23] elements (64 rows stay below 2^31 bytes)
bool operand_ok(const void* p, const long* s) {
  return p && s && (((uintptr_t)p) & 15) == 0 && s[0] % 8 == 0 && s[1] % 8 == 0 && s[2] % 8 == 0 && s[1] >= 0 &&
         s[1] <= (1L << 23);
}

// What a call launches, from its numbers alone: shapes, strides and addresses (for their alignment)
// are read, nothing is dereferenced and no HIP function is called.  bwd: ops holds q, k, v, o, dout,
// dq, dk, dv and their strides; fwd: q, k, v, o.
Plan128 plan128(bool bwd, const void* const* ops, const long* const* st, const void* lse, int B, int Sq, int Sk, int H,
                int Hkv, int causal) {
  Plan128 p = {hipErrorInvalidValue, kFwd0, 0, 256};
  if (B <= 0 || Sq <= 0 || Sk <= 0 || H <= 0 || Hkv <= 0 || H % Hkv != 0) return p;
  if (!lse || (((uintptr_t)lse) & 3)) return p;
  for (int i = 0; i < (bwd ? 8 : 4); ++i)
    if (!operand_ok(ops[i], st[i])) return p;
  const long nqb = (Sq + QB - 1) / QB, nkt = (Sk + BLK - 1) / BLK;
  const long grid = nqb * H * B + (bwd ? nkt * Hkv * B : 0);
  if (grid >= (1L << 30) || (long)H * B >= (1L << 30)) return p;
  const bool mask = causal || Sk % BLK != 0;
  p.err = hipSuccess;
  p.inst = bwd ? (mask ? kBwd1 : kBwd0) : (mask ? kFwd1 : kFwd0);
  p.grid = (unsigned)grid;
  return p;
}

void set_strides(long& sb, long& ss, long& sh, const long* s) {
  sb = s[0]; ss = s[1]; sh = s[2];
}
Attn128Args args128(const void* q, const void* k, const void* v, const void* o, void* lse, const long* qs,
                    const long* ks, const long* vs, const long* os, int B, int Sq, int Sk, int H, int Hkv, float scale,
                    int causal, int q_offset) {
  Attn128Args a = {};
  a.q = (const bf16_t*)q; a.k = (const bf16_t*)k; a.v = (const bf16_t*)v; a.o = (const bf16_t*)o;
  a.lse = (float*)lse;
  set_strides(a.q_sb, a.q_ss, a.q_sh, qs);
  set_strides(a.k_sb, a.k_ss, a.k_sh, ks);
  set_strides(a.v_sb, a.v_ss, a.v_sh, vs);
  set_strides(a.o_sb, a.o_ss, a.o_sh, os);
  a.B = B; a.Sq = Sq; a.Sk = Sk; a.H = H; a.Hkv = Hkv; a.G = H / Hkv;
  a.nqb = (Sq + QB - 1) / QB;
  a.nkt = (Sk + BLK - 1) / BLK;
  a.scale = scale; a.scale_log2 = scale * LOG2E;
  a.causal = causal; a.q_offset = q_offset;
  return a;
}

int fwd128(const void* q, const void* k, const void* v, void* o, void* lse, int B, int Sq, int Sk, int H, int Hkv,
           const long* qs, const long* ks, const long* vs, const long* os, float scale, int causal, int q_offset,
           hipStream_t stream, Plan128* plan) {
  const void* ops[4] = {q, k, v, o};
  const long* st[4] = {qs, ks, vs, os};
  const Plan128 p = plan128(false, ops, st, lse, B, Sq, Sk, H, Hkv, causal);
  if (plan) *plan = p;
  if (plan || p.err != hipSuccess) return (int)p.err;
  Attn128Args a = args128(q, k, v, o, lse, qs, ks, vs, os, B, Sq, Sk, H, Hkv, scale, causal, q_offset);
  a.out = (bf16_t*)o;
  const dim3 grid(p.grid), block(p.block);
  ljs_launch_rec(kInstName[p.inst], grid, p.block);
  if (p.inst == kFwd1) hipLaunchKernelGGL(attn128_fwd_kernel<true>, grid, block, 0, stream, a);
  else hipLaunchKernelGGL(attn128_fwd_kernel<false>, grid, block, 0, stream, a);
  return (int)hipGetLastError();
}

int bwd128(const void* q, const void* k, const void* v, const void* o, const void* dout, const void* lse, void* dq,
           void* dk, void* dv, int B, int Sq, int Sk, int H, int Hkv, const long* qs, const long* ks, const long* vs,
           const long* os, const long* dos, const long* dqs, const long* dks, const long* dvs, float scale, int causal,
           int q_offset, hipStream_t stream, Plan128* plan) {
  const void* ops[8] = {q, k, v, o, dout, dq, dk, dv};
  const long* st[8] = {qs, ks, vs, os, dos, dqs, dks, dvs};
  const Plan128 p = plan128(true, ops, st, lse, B, Sq, Sk, H, Hkv, causal);
  if (plan) *plan = p;
  if (plan || p.err != hipSuccess) return (int)p.err;
  Attn128Args a = args128(q, k, v, o, (void*)lse, qs, ks, vs, os, B, Sq, Sk, H, Hkv, scale, causal, q_offset);
  a.dout = (const bf16_t*)dout;
  a.dq = (bf16_t*)dq; a.dk = (bf16_t*)dk; a.dv = (bf16_t*)dv;
  set_strides(a.do_sb, a.do_ss, a.do_sh, dos);
  set_strides(a.dq_sb, a.dq_ss, a.dq_sh, dqs);
  set_strides(a.dk_sb, a.dk_ss, a.dk_sh, dks);
  set_strides(a.dv_sb, a.dv_ss, a.dv_sh, dvs);
  const dim3 grid(p.grid), block(p.block);
  ljs_launch_rec(kInstName[p.inst], grid, p.block);
  if (p.inst == kBwd1) hipLaunchKernelGGL(attn128_bwd_kernel<true>, grid, block, 0, stream, a);
  else hipLaunchKernelGGL(attn128_bwd_kernel<false>, grid, block, 0, stream, a);
  return (int)hipGetLastError();
}

}  // namespace

// o [B][Sq][H][128] bf16 and lse [B][H][Sq] f32 of q [B][Sq][H][128], k / v [B][Sk][Hkv][128]; strides in
// elements, ordered (batch, seq, head), the head dim contiguous.  What the plan rejects (a null operand,
// H % Hkv != 0, a non-positive size, 2^30 blocks or more, a base or stride off the 16-byte grid, a
// sequence stride outside [0, 2^23]) returns hipErrorInvalidValue with nothing launched or recorded.
LJS_API int ljs_attn128_fwd(const void* q, const void* k, const void* v, void* o, void* lse, int B, int Sq, int Sk,
                            int H, int Hkv, const long* qs, const long* ks, const long* vs, const long* os, float scale,
                            int causal, int q_offset, hipStream_t stream) {
  return fwd128(q, k, v, o, lse, B, Sq, Sk, H, Hkv, qs, ks, vs, os, scale, causal, q_offset, stream, nullptr);
}
// dq [B][Sq][H][128], dk / dv [B][Sk][Hkv][128] (already summed over each group's query heads) of the
// keys k / v alone, given the final o and the lse of the whole attention; no workspace
LJS_API int ljs_attn128_bwd(const void* q, const void* k, const void* v, const void* o, const void* dout,
                            const void* lse, void* dq, void* dk, void* dv, int B, int Sq, int Sk, int H, int Hkv,
                            const long* qs, const long* ks, const long* vs, const long* os, const long* dos,
                            const long* dqs, const long* dks, const long* dvs, float scale, int causal, int q_offset,
                            hipStream_t stream) {
  return bwd128(q, k, v, o, dout, lse, dq, dk, dv, B, Sq, Sk, H, Hkv, qs, ks, vs, os, dos, dqs, dks, dvs, scale,
                causal, q_offset, stream, nullptr);
}
// The plan of ljs_attn128_fwd (kind 0) / ljs_attn128_bwd (kind 1) without a GPU.  addr: q, k, v, o,
// lse, dout, dq, dk, dv; st: the (batch, seq, head) strides of q, k, v, o, dout, dq, dk, dv.  out[0..3]:
// error, launches, grid, block; name: the launch record's name.  Returns the error.
LJS_API int ljs_attn128_plan(int kind, int B, int Sq, int Sk, int H, int Hkv, int causal, void* const* addr,
                             const long* st, int* out, char* name, int cap) {
  Plan128 p = {hipErrorInvalidValue, kFwd0, 0, 256};
  if (addr && st) {
    void* const* x = addr;
    if (kind == 0)
      fwd128(x[0], x[1], x[2], x[3], x[4], B, Sq, Sk, H, Hkv, st, st + 3, st + 6, st + 9, 1.f, causal, 0, nullptr, &p);
    else if (kind == 1)
      bwd128(x[0], x[1], x[2], x[3], x[5], x[4], x[6], x[7], x[8], B, Sq, Sk, H, Hkv, st, st + 3, st + 6, st + 9,
             st + 12, st + 15, st + 18, st + 21, 1.f, causal, 0, nullptr, &p);
  }
  const bool ok = p.err == hipSuccess;
  out[0] = (int)p.err; out[1] = ok; out[2] = (int)p.grid; out[3] = (int)p.block;
  if (name && cap > 0) snprintf(name, (size_t)cap, "%s", ok ? kInstName[p.inst] : "");
  return (int)p.err;
}
