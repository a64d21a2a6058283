// LJS_HIPCC_FLAGS: -Xclang -target-feature -Xclang -packed-fp32-ops -mllvm -amdgpu-mfma-vgpr-form
// Chunked prefill: flash-style MFMA attention of T >= 1 new positions per sequence over the KV cache
// buffers themselves (head_dim 64, bf16 q and o; bf16 or MX-fp8 caches).
//
// Semantics (ops/kernels.py, attn_chunk_reference).  q is (B, T, H, 64), kc / vc are (B, cap, Hkv, 64), lens
// is int32 [B] ON THE DEVICE.  A kv_append has just written the T positions at rows lens[b] .. lens[b] +
// T - 1, which lens does not count yet.  Row (b, t, h) attends to the cache rows [0, n), n = clamp(lens[b]
// + t + 1, 0, cap), of key/value head h / G (G = H / Hkv):
//     o[b][t][h]    = bf16( sum_key bf16(p[key]) vc[b][key][h / G] / l ),  p = exp2(s scale log2e - m)
//     lse2[b][t][h] = m + log2(l)
// and n = 0 gives o = 0, lse2 = +inf.  f32 scores, the scale folded into the exp2 argument, a running
// max, probabilities rounded to bf16 before P.V, f32 accumulation, one rounding of O: attention.hip's
// forward.  No kernel argument depends on lens, so a captured launch stays valid as sequences grow.
//
// Rows and grid.  A row is a (t, g) pair of one (batch, key/value head), r = t G + g, G any value in
// 1..16.  One block of 4 waves takes ROWS consecutive rows: 128 (32 per wave as two 16-row MFMA chains
// that share every K and V fragment) or 64 (16 per wave).  All heads of a group ride on the M side, so a
// K/V tile is fetched once per key/value head, and the rows of a block have nearly equal key limits:
// the masked region is a thin band at the end of the sweep.  The grid is (row tiles, Hkv, B), of T, H
// and Hkv only; block x takes row tile (tiles - 1 - x), so the latest positions (the longest sweeps)
// start first.
//
// Scores.  S^T = K . Q^T with the 16x16x32 bf16 MFMA: a lane owns one row (the accumulator column) and 16
// of a tile's 64 keys, so the row's key limit is one in-lane compare and the softmax stays in-lane but
// for two lane swaps.  Q fragments go from global memory straight to registers.  P^T leaves the
// accumulators, rounded to bf16, as the B operand of O^T = V^T . P^T, V^T coming from the transposing
// LDS read.
//
// Key sweep.  64-key tiles in ascending order from row 0 up to the block's largest limit (one scalar
// load of lens[b]).  A wave runs the unmasked tile body while the tile ends at or below the smallest
// limit of its rows, the masked body over the boundary band, and nothing beyond its largest limit.  K
// and V are read through buffer descriptors that end with the block's last live row: rows past it read
// as zeros whatever the memory holds, and a row's own limit is applied by a select in front of the
// exp2, so a poisoned row never reaches arithmetic.
//
// bf16 cache: the tiles go by LDS-DMA (the swizzle on the source address) into [64][64] bf16 images,
// 16-byte chunk c of row r at c ^ 2 ((r >> 1) & 3): conflict-free for the ds_read_b128 operand reads
// and the ds_read_b64_tr_b16 transposing reads.  Two stages of (K, V), 32 KiB, one barrier per tile.
// MX-fp8 cache (e4m3 bytes (B, cap, Hkv, 64), e8m0 scales (B, cap, Hkv, 2), strides in bytes): a lane
// loads 16 bytes of K, 16 of V and their scale bytes of the NEXT tile into VGPRs while the current tile
// computes, converts them with the scaled conversion (exact: 4 significant bits times a power of two;
// a zero scale byte is 2^-127) and writes the same bf16 image with ds_write_b128.  From there on the
// sweep is the bf16 instance's instruction for instruction: attn_chunk_q8 on a cache has the bits of
// attn_chunk on its dequantised copy.
//
// Output.  The ring is idle after the sweep: a wave stages its rows in 2 or 4 KiB of it and they leave
// as whole 128-byte rows.  No atomics, no memset, no workspace, no tickets; the same bits on every run.
//
// Entry point.  ljs_attn_chunk takes the cache as one LjsCache descriptor with an explicit kind
// (cache_common.h: the struct, the alignment rules and the reach check decode.hip's launchers use too).
#include "cache_common.h"
#include "common.h"

namespace {

constexpr int kD = 64;                  // head dim
constexpr int kKeys = 64;               // keys per tile
constexpr int kImg = kKeys * kD;        // elements of one LDS image (8 KiB)
constexpr int kThreads = 256;
constexpr int kMaxG = 16;
constexpr float kLog2e = 1.4426950408889634f;

int g_chunk_rows = 0;                   // 64 / 128: a tile forced by tests

struct ChunkArgs {
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

// ---- the LDS image: element index of 16-byte chunk c16 / 8-byte piece c8 of a row
__device__ __forceinline__ int swz(int row) { return ((row >> 1) & 3) << 1; }
__device__ __forceinline__ int img16(int row, int c16) { return row * kD + ((c16 ^ swz(row)) << 3); }
__device__ __forceinline__ int img8(int row, int c8) { return img16(row, c8 >> 1) + ((c8 & 1) << 2); }

// The lane parts of the fragment addresses, once per kernel: the swizzle reads bits 1..2 of the row
// number only, so a row base that is a multiple of 8 is an immediate offset on top of them.
struct LaneOff {
  int rows[2];   // img16(lane & 15, 4 ks + (lane >> 4)): the ds_read_b128 operand of k-step ks
  int tr[4];     // img8(4 (lane >> 4) + ((lane & 15) >> 2), 4 dt + (lane & 3)): the transposed operand of d tile dt
};
__device__ __forceinline__ LaneOff lane_off(int lane) {
  LaneOff f;
  const int i = lane & 15, g = lane >> 4;
#pragma unroll
  for (int ks = 0; ks < 2; ++ks) f.rows[ks] = img16(i, 4 * ks + g);
#pragma unroll
  for (int dt = 0; dt < 4; ++dt) f.tr[dt] = img8(4 * g + (i >> 2), 4 * dt + (i & 3));
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
  f32x4 o[4];    // O^T: d 16 dt + 4 (lane >> 4) + e of row lane & 15
  float m, l;    // the running max (all 4 lanes of a row agree) and this lane's part of the sum
};

// One 64-key tile for a wave's CH chains of 16 rows.  MASK: a score whose key is at or beyond its row's
// limit nr[c] is replaced by -inf before anything reads it.
template <int CH, bool MASK>
__device__ __forceinline__ void chunk_tile(RowState (&st)[CH], const bf16_t* Kt, const bf16_t* Vt,
                                           const bf16x8 (&qf)[CH][2], const int (&nr)[CH], int kbase, float sl2,
                                           int lane, const LaneOff& f) {
  const int g = lane >> 4;
  f32x4 s[CH][4];
#pragma unroll
  for (int jt = 0; jt < 4; ++jt) {
    const bf16x8 k0 = frag_k(Kt, jt, 0, f), k1 = frag_k(Kt, jt, 1, f);
#pragma unroll
    for (int c = 0; c < CH; ++c) {
      s[c][jt] = mfma16x16x32(k0, qf[c][0], f32x4{0.f, 0.f, 0.f, 0.f});
      s[c][jt] = mfma16x16x32(k1, qf[c][1], s[c][jt]);
    }
  }
  u32x4 pb[CH][2];
#pragma unroll
  for (int c = 0; c < CH; ++c) {
    if constexpr (MASK) {
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
    float m_use = m_new;
    if constexpr (MASK) m_use = m_new == -INFINITY ? 0.f : m_new;   // no key seen so far: p = 0
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
      for (int dt = 0; dt < 4; ++dt) st[c].o[dt] = st[c].o[dt] * alpha;
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
    for (int dt = 0; dt < 4; ++dt) {
      const bf16x8 va = frag_vt(Vt, 32 * s2, dt, f);
#pragma unroll
      for (int c = 0; c < CH; ++c) st[c].o[dt] = mfma16x16x32(va, __builtin_bit_cast(bf16x8, pb[c][s2]), st[c].o[dt]);
    }
}

// bf16 cache: rows kb0 .. kb0 + 63 of one (batch, key/value head) slab into an image by LDS-DMA, 8 pieces
// of 8 rows x 128 bytes, two per wave.  The resource is rebased on the tile and ends with live row n_end
// - 1: rows at and beyond n_end land as zeros.  ld: the row stride in bytes.
__device__ __forceinline__ void dma_tile(const unsigned char* base, long ld, int kb0, int n_end, bf16_t* img, int wave,
                                         int lane) {
  const int nr = n_end - kb0 < kKeys ? n_end - kb0 : kKeys;
  const u32x4 rs = rsrc_u4(base + (long)kb0 * ld, (long)(nr - 1) * ld + 2 * kD);
  const int ld32 = (int)ld;
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    const int pc = wave + 4 * i, row = 8 * pc + (lane >> 3);
    const int c = (lane & 7) ^ swz(row);
    dma_lds_x4(rs, row < nr ? row * ld32 + c * 16 : 0x7ffffff0, img + pc * 512);
  }
}

// MX-fp8 cache: a lane's quarter row (16 elements inside one scale block) of K and of V, on its way from
// the descriptors (which end with the block's last live row) to the bf16 images
struct Q8Regs {
  u32x4 k, v;
  unsigned ke, ve;
  __device__ __forceinline__ void load(const __amdgpu_buffer_rsrc_t& rk, const __amdgpu_buffer_rsrc_t& rv,
                                       const __amdgpu_buffer_rsrc_t& rks, const __amdgpu_buffer_rsrc_t& rvs,
                                       const ChunkArgs& a, int kb0, int tid) {
    const int row = kb0 + (tid >> 2), qr = tid & 3;
    k = __builtin_amdgcn_raw_buffer_load_b128(rk, row * (int)a.ks + qr * 16, 0, 0);
    v = __builtin_amdgcn_raw_buffer_load_b128(rv, row * (int)a.vs + qr * 16, 0, 0);
    ke = __builtin_amdgcn_raw_buffer_load_b8(rks, row * (int)a.kss + (qr >> 1), 0, 0);
    ve = __builtin_amdgcn_raw_buffer_load_b8(rvs, row * (int)a.vss + (qr >> 1), 0, 0);
  }
  static __device__ __forceinline__ void put(bf16_t* img, const u32x4& x, unsigned e, int tid) {
    const float sf = __uint_as_float(e << 23);     // 2^(e - 127); the conversion reads the exponent field (0: 2^-127)
    unsigned w[8];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      w[2 * i] = __builtin_bit_cast(unsigned, __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(x[i], sf, false));
      w[2 * i + 1] = __builtin_bit_cast(unsigned, __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(x[i], sf, true));
    }
    const int row = tid >> 2, qr = tid & 3;
    *reinterpret_cast<u32x4*>(img + img16(row, 2 * qr)) = u32x4{w[0], w[1], w[2], w[3]};
    *reinterpret_cast<u32x4*>(img + img16(row, 2 * qr + 1)) = u32x4{w[4], w[5], w[6], w[7]};
  }
  __device__ __forceinline__ void store(bf16_t* stage, int tid) const {
    put(stage, k, ke, tid);
    put(stage + kImg, v, ve, tid);
  }
};

// A lane's 16 d-values of local row rbase + (lane & 15) into a wave-private [rows][64] bf16 image (16-byte
// chunk c of row r at c ^ (r & 7)), and NR staged rows out as whole 128-byte rows, 8 per store
// instruction; row r0 + i of the block is (t, g) = (r / G, r % G).
__device__ __forceinline__ void stage_rows16(bf16_t* img, int rbase, const f32x4 (&acc)[4], float mul, int lane) {
  const int r = rbase + (lane & 15), g = lane >> 4;
#pragma unroll
  for (int dt = 0; dt < 4; ++dt) {
    u32x2 w;
    w[0] = pack_bf16x2(acc[dt][0] * mul, acc[dt][1] * mul);
    w[1] = pack_bf16x2(acc[dt][2] * mul, acc[dt][3] * mul);
    const int c = (2 * dt + (g >> 1)) ^ (r & 7);
    *reinterpret_cast<u32x2*>(img + r * kD + c * 8 + 4 * (g & 1)) = w;
  }
}
template <int NR>
__device__ __forceinline__ void flush_rows(const bf16_t* img, bf16_t* base, const ChunkArgs& a, int r0, int R, int h0,
                                           int lane) {
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");   // this wave's image writes are done (wave-private)
  u32x4 v[NR / 8];
#pragma unroll
  for (int i = 0; i < NR / 8; ++i) {
    const int r = 8 * i + (lane >> 3), c = lane & 7;
    v[i] = *reinterpret_cast<const u32x4*>(img + r * kD + ((c ^ (r & 7)) << 3));
  }
#pragma unroll
  for (int i = 0; i < NR / 8; ++i) {
    const int r = r0 + 8 * i + (lane >> 3), c = lane & 7;
    if (r < R) {
      const int t = r / a.G, g = r - t * a.G;
      *reinterpret_cast<u32x4*>(base + (long)t * a.ot + (long)(h0 + g) * a.oh + c * 8) = v[i];
    }
  }
}

template <int ROWS, bool MX8>
__global__ __launch_bounds__(kThreads, 2) void attn_chunk_kernel(const ChunkArgs a) {
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

  bf16x8 qf[CH][2];
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
    for (int ks = 0; ks < 2; ++ks)
      qf[c][ks] = __builtin_bit_cast(bf16x8, ok[c] ? *reinterpret_cast<const u32x4*>(qp + 32 * ks) : u32x4{0u, 0u, 0u, 0u});
#pragma unroll
    for (int i = 0; i < 4; ++i) st[c].o[i] = f32x4{0.f, 0.f, 0.f, 0.f};
    st[c].m = -INFINITY;
    st[c].l = 0.f;
  }

  const unsigned char* kbp = a.kc + (long)b * a.kb + (long)j * a.kh;
  const unsigned char* vbp = a.vc + (long)b * a.vb + (long)j * a.vh;
  // MX8: descriptors over the whole live range (a row is 64 bytes and 2 scale bytes)
  __amdgpu_buffer_rsrc_t rk, rv, rks, rvs;
  Q8Regs regs;
  if constexpr (MX8) {
    rk = make_rsrc(kbp, n_max > 0 ? (long)(n_max - 1) * a.ks + kD : 0);
    rv = make_rsrc(vbp, n_max > 0 ? (long)(n_max - 1) * a.vs + kD : 0);
    rks = make_rsrc(a.ksc + (long)b * a.ksb + (long)j * a.ksh, n_max > 0 ? (long)(n_max - 1) * a.kss + 2 : 0);
    rvs = make_rsrc(a.vsc + (long)b * a.vsb + (long)j * a.vsh, n_max > 0 ? (long)(n_max - 1) * a.vss + 2 : 0);
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
    if (kbase < w_hi) {
      if (kbase + kKeys <= w_lo) chunk_tile<CH, false>(st, Kt, Kt + kImg, qf, nr, kbase, a.scale_log2, lane, f);
      else chunk_tile<CH, true>(st, Kt, Kt + kImg, qf, nr, kbase, a.scale_log2, lane, f);
    }
    if constexpr (MX8) {
      if (more) regs.store(smem + ((kt + 1) & 1) * 2 * kImg, tid);
    }
  }
  __syncthreads();   // the ring is idle: this wave's rows of O leave through WR x 128 bytes of it
  if (!wave_live) return;
  bf16_t* img = smem + wave * WR * kD;
#pragma unroll
  for (int c = 0; c < CH; ++c) {
    const float lt = row4_sum(st[c].l);
    if ((lane >> 4) == 0 && ok[c])
      a.lse[((long)b * a.T + trow[c]) * a.H + h0 + grow[c]] = lt > 0.f ? st[c].m + __log2f(lt) : INFINITY;
    stage_rows16(img, 16 * c, st[c].o, lt > 0.f ? 1.f / lt : 0.f, lane);
  }
  flush_rows<WR>(img, a.o + (long)b * a.ob, a, r0w, R, h0, lane);
}

// ---- the plan: pure, of the shape and the CU count, never of the lengths.  128-row tiles, or 64-row
// tiles when the rows of a group fit one of them or 128-row tiles would leave compute units idle.
inline void plan_chunk(int B, int T, int H, int Hkv, int cus, int* rows, unsigned* grid) {
  const long R = (long)T * (H / Hkv);
  const long blocks128 = ((R + 127) / 128) * Hkv * B;
  *rows = (R <= 64 || blocks128 < cus) ? 64 : 128;
  grid[0] = (unsigned)((R + *rows - 1) / *rows);
  grid[1] = (unsigned)Hkv;
  grid[2] = (unsigned)B;
}

// the launch of ljs_attn_chunk over a cache of the template's kind (c.kind has chosen it)
template <bool MX8>
int chunk_launch(const void* q, const LjsCache& c, void* o, void* lse, const void* lens, int B, int T, int H,
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
  ChunkArgs a{};
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
  int rows;
  unsigned g[3];
  plan_chunk(B, T, H, Hkv, ljs_device_cus(), &rows, g);
  if (g_chunk_rows) {
    rows = g_chunk_rows;
    g[0] = (unsigned)(((long)T * a.G + rows - 1) / rows);
  }
  const dim3 grid(g[0], g[1], g[2]);
  if (rows == 128) hipLaunchKernelGGL((attn_chunk_kernel<128, MX8>), grid, dim3(kThreads), 0, st, a);
  else hipLaunchKernelGGL((attn_chunk_kernel<64, MX8>), grid, dim3(kThreads), 0, st, a);
  ljs_launch_rec(rows == 128 ? (MX8 ? "attn_chunk<R128,mx8>" : "attn_chunk<R128>")
                             : (MX8 ? "attn_chunk<R64,mx8>" : "attn_chunk<R64>"), grid, kThreads);
  return (int)hipGetLastError();
}

}  // namespace

// tests: force 64- or 128-row tiles, here and in prefill128.hip (which reads it back); anything else restores the plan
LJS_API int ljs_chunk_set_rows(int n) {
  g_chunk_rows = (n == 64 || n == 128) ? n : 0;
  return 0;
}
LJS_API int ljs_chunk_get_rows() { return g_chunk_rows; }

// out = {rows, grid x, y, z} of (B, T, H, Hkv) on a device of `cus` compute units: pure
LJS_API int ljs_chunk_plan(int B, int T, int H, int Hkv, int cus, int* out) {
  if (B < 1 || T < 1 || H < 1 || Hkv < 1 || cus < 1 || H % Hkv != 0 || !out) return (int)hipErrorInvalidValue;
  unsigned g[3];
  plan_chunk(B, T, H, Hkv, cus, out, g);
  out[1] = (int)g[0]; out[2] = (int)g[1]; out[3] = (int)g[2];
  return 0;
}

// q (B, T, H, 64) over the cache c (cache_common.h; either kind) -> o (B, T, H, 64) bf16, lse (B, T, H) f32: row (b, t, h)
// over the cache rows [0, clamp(lens[b] + t + 1, 0, cap)) (the head of the file).  sq / so: (batch, position, head) strides
// in elements.  One launch.  Returns hipErrorInvalidValue, and launches and records nothing, for an empty
// shape, H % Hkv != 0, H / Hkv > 16, scale <= 0, a null or misaligned lens or lse, a base or stride of q or o
// that is not 16-byte aligned, or a cache cache_aligned or cache_reach_ok refuses (a kind that does not match
// its scale bases, a misaligned buffer, a key stride below 64 or a scale row stride below 2, byte offsets that
// do not fit 31 bits), or a cache whose head dim is not 64 (the kernel exists at 64 only).
LJS_API int ljs_attn_chunk(const void* q, const LjsCache* c, void* o, void* lse, const void* lens, int B, int T, int H,
                           const long* sq, const long* so, float scale, hipStream_t st) {
  if (!c || c->dim != 64) return (int)hipErrorInvalidValue;
  return c->kind == kCacheMx8 ? chunk_launch<true>(q, *c, o, lse, lens, B, T, H, sq, so, scale, st)
                              : chunk_launch<false>(q, *c, o, lse, lens, B, T, H, sq, so, scale, st);
}
