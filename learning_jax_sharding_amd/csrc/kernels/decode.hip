// Decoding with a key/value cache: the cache append (with the rotary embedding of the new q and k at
// a position read on the device) and single-query split-K attention over the cache.
//
// Layout.  q is (B, T, H, 64), new k / v are (B, T, Hkv, 64), the caches kc / vc are (B, cap, Hkv, 64),
// all bf16 with the head dim contiguous and their own (batch, position, head) strides in elements
// (column blocks of a fused projection buffer are read in place); every base and stride is 16-byte
// aligned and offsets are 64-bit.  lens is int32 [B] ON THE DEVICE: no kernel argument depends on the
// current lengths, so a launch captured into a graph stays valid while the sequences grow.  Query
// head h reads key/value head h / G, G = H / Hkv (attention.hip's convention).
//
// kv_append.  With p = base[b] + t, base[b] = lens[b] (decode) or 0 when lens is null (prefill):
//     vc[b][p] = v[b][t]                      (the 16-byte chunks as they are)
//     kc[b][p] = rot(k[b][t], p)              (or k[b][t] as it is without a table)
//     q_out[b][t] = rot(q[b][t], p)           (optional)
// rot is rope.hip's map: the same f32 cos / sin table, the same half-split pairs and the same f32
// expressions, so the bits are rope_kernel's at position p.  Rows with p outside [0, cap) are not
// written to the caches (q_out gets zeros there).  One work item is (tensor, batch, t, head, j): the
// chunks j and j + 4 of one head row (the two halves' matching 8 elements), grid-stride over a grid
// sized from the CU count.  No LDS, no cross-lane traffic, no atomics.
//
// attn_decode.  For sequence b the keys are the rows [0, n_b), n_b = min(lens[b] + extra, cap) (extra
// = 1 after an append that lens does not count yet):
//     o[b][0][h]  = bf16( sum_key bf16(p[key]) vc[b][key][h / G] / l ),  p = exp2(s scale log2e - m)
//     lse2[b][h]  = m + log2(l)          (log2 of the partition function of the scaled scores)
// and n_b = 0 gives o = 0, lse2 = +inf.  f32 scores, the scale folded into the exp2 argument, a running
// max, probabilities rounded to bf16 before P.V, f32 accumulation, one rounding of O: the forward of
// attention.hip.  The key axis is cut into `splits` ranges of `keys_per_split` keys by a pure plan
// (plan_decode: of B, Hkv, cap and the CU count, never of the lengths); the grid is splits x Hkv x B
// and a block whose range starts at or beyond n_b writes the empty partial (m = -inf, l = 0, acc = 0).
//
// One block of 4 waves takes one (batch, key/value head, split) and ALL G <= 16 query heads of the
// group, so a K/V byte is fetched once per key/value head.  A key row is 8 chunks of 16 bytes: 8
// lanes hold one key, a wave 8 keys per step, and every lane keeps its chunk's 8 columns of q and of
// the accumulator of each head.  K and V go straight from memory to VGPRs (kDecUnroll steps of
// buffer loads are issued before the first is used; no LDS staging); a score is 4 packed bf16 dot
// products and a 3-step DPP sum over the key's 8 lanes, after which all 8 lanes hold it.  A wave
// carries at most 8 heads (registers): for G > 8 waves 0-1 take heads 0..7 and waves 2-3 heads 8..15,
// each pair sweeping the whole range (the second pair's loads hit the cache).  Every 8-lane slot runs
// its own online softmax; the 8 slots of a wave are merged by shuffles and the waves through 9 KiB of
// LDS, both in a fixed order.
//
// Rows at and beyond the end of a block's range never reach a register: K and V are read through
// buffer descriptors that end with the last row of the range, so a load past it returns zeros
// whatever the memory holds (NaN, Inf), and its score is replaced by -inf.
//
// splits == 1: the block writes o and lse2 itself.  Otherwise the partials (m, l, acc[64] per head,
// f32) go to a workspace and a second small launch (decode_merge, one wave per (b, h)) merges them in
// a fixed order -- eight interleaved chains, each in ascending split order, then a fixed tree: the
// same bits on every run.  (The in-launch last-arriver form of rowwise.h would save that
// launch, about 2 us inside a graph, at the price of write-through stores, a ticket per (b, kv head) and
// a serial merge tail in whichever block arrives last; with a kernel boundary in between, plain
// stores are enough.)
//
// attn_extend (ljs_attn_extend, ljs_attn_extend_q8).  q is (B, T, H, 64), 1 <= T <= 64 positions per sequence that
// a kv_append has just written at rows lens[b] .. lens[b] + T - 1 and lens does not count yet: row (b, t, h)
// attends to the rows [0, clamp(lens[b] + t + 1, 0, cap)) and gets the bits attn_decode writes for (b, h) with
// extra = t + 1 under the same plan (the same kernel, its EXT instances: a wave's heads become rows (t, g)
// with a key limit each; the comment at the kernel).  A block carries all G heads of 8 / G positions (one
// for G > 4), the row tiles sit beside the splits in grid.x, the partials and decode_merge are reused with
// B T H outputs, and T == 1 launches attn_decode's own instances.
//
// MX-fp8 caches (the mx8 instances; ljs_kv_append_q8, ljs_attn_decode_q8).  kc / vc hold OCP e4m3 bytes (B,
// cap, Hkv, 64) and two more buffers one e8m0 byte per 32 elements (B, cap, Hkv, 2), in the encoding
// ljs_quant_mx_rows writes (exponent + 127); strides of all four count bytes.  The append stores
// quantize_mx_ref of the bf16 row the bf16 cache would hold (rope's bits first, then the quantiser;
// kv_append_q8_kernel), the attention is the bf16 attention over the dequantised rows, which are exact
// bf16 values (attn_decode_kernel<HW, true>: the same grid, plan, partials and merge; only the loads and
// two scaled conversions per 4 elements differ).  A zero scale byte is 2^-127, as for dequantize_mx_ref and the
// block-scaled MFMA: a live row whose block exponent clamped carries it with non-zero bytes.  Rows beyond a
// block's range read zero bytes (and a zero scale byte) through the descriptors: 0 x 2^-127 = 0.
#include "rowwise.h"

namespace {

constexpr int kDecD = 64;                 // head dim
constexpr int kDecChunks = kDecD / 8;     // 16-byte chunks per head row = lanes per key
constexpr int kDecThreads = 256;
constexpr int kDecWaves = kDecThreads / 64;
constexpr int kDecSlots = 64 / kDecChunks;             // keys a wave holds per step
constexpr int kDecKeyTile = kDecWaves * kDecSlots;     // keys a block holds per step: 32
constexpr int kDecUnroll = 4;             // steps whose loads are in flight together (8 measured slower at
                                          // one head per wave: 119.7 against 112.6 us at B = 64, 4096 keys)
constexpr int kDecWaveHeads = 8;          // query heads one wave carries
constexpr int kDecMaxG = 2 * kDecWaveHeads;
constexpr int kExtMaxT = 64;              // query positions per sequence one attn_extend call takes
constexpr int kDecPart = 72;              // floats of one partial: acc[64], m, l, padded to 16 bytes
constexpr int kDecBlocksPerCu = 4;        // the plan's target: blocks per compute unit
constexpr int kDecMinTiles = 8;           // a split sweeps at least 8 key tiles (256 keys), 4 on an unfilled chip
constexpr int kDecOneSplitTiles = 16;     // up to 512 rows of capacity: one split (no merge launch)
constexpr int kAppBlocksPerCu = 8;

int g_dec_splits = 0, g_dec_keys = 0;     // > 0: a plan forced by tests

__device__ __forceinline__ float dec_exp2(float x) { return __builtin_amdgcn_exp2f(x); }

template <int CTRL>
__device__ __forceinline__ float dpp_mov(float v) {
  return __uint_as_float((unsigned)__builtin_amdgcn_update_dpp(0, (int)__float_as_uint(v), CTRL, 0xf, 0xf, false));
}
// sum over the 8 lanes of a key; every one of them ends up with the same bits (each step adds the
// same two numbers in both partners)
__device__ __forceinline__ float sum8(float v) {
  v += dpp_mov<0xB1>(v);    // quad_perm [1,0,3,2]
  v += dpp_mov<0x4E>(v);    // quad_perm [2,3,0,1]
  v += dpp_mov<0x141>(v);   // row_half_mirror: lane i <-> 7 - i, the other quad
  return v;
}

__device__ __forceinline__ float dot2_bf16(unsigned a, unsigned b, float c) {
#if __has_builtin(__builtin_amdgcn_fdot2_f32_bf16)
  return __builtin_amdgcn_fdot2_f32_bf16(__builtin_bit_cast(bf16x2_t, a), __builtin_bit_cast(bf16x2_t, b), c, false);
#else
  return fmaf(bf16_hi(a), bf16_hi(b), fmaf(bf16_lo(a), bf16_lo(b), c));
#endif
}

// (m, l, acc) <- merged with (m2, l2, acc2): log-sum-exp in the log2 domain; m = -inf is "no key yet"
__device__ __forceinline__ void dec_merge(float& m, float& l, float (&acc)[8], float m2, float l2,
                                          const float (&acc2)[8]) {
  const float mn = fmaxf(m, m2);
  const float mu = mn == -INFINITY ? 0.f : mn;
  const float a1 = dec_exp2(m - mu), a2 = dec_exp2(m2 - mu);
  l = l * a1 + l2 * a2;
#pragma unroll
  for (int e = 0; e < 8; ++e) acc[e] = acc[e] * a1 + acc2[e] * a2;
  m = mn;
}

struct DecodeArgs {
  const bf16_t *q, *kc, *vc;
  bf16_t* o;
  float* lse;                 // [B][H]
  float* ws;                  // [B][H][splits][kDecPart]
  const int* lens;
  long qb, qh;                // strides (elements): batch, head (one position)
  long kb, ks, kh, vb, vs, vh, ob, oh;
  int B, H, Hkv, G, cap, extra, splits, kps;
  float scale_log2;
  // attn_extend only (T = 1, P = 1 otherwise): the position strides of q and o, the query positions per
  // sequence and the positions one block carries
  long qt, ot;
  int T, P;
  // MX-fp8 caches only (kc / vc are then e4m3 bytes and their strides count bytes): the e8m0 scales
  // (B, cap, Hkv, 2) and their (batch, position, head) strides in bytes
  const unsigned char *ksc, *vsc;
  long ksb, kss, ksh, vsb, vss, vsh;
};

// final output of one (b, t, h, chunk) from a merged state: o is the row's first element, lse its entry
__device__ __forceinline__ void dec_store_out(bf16_t* o, float* lse, int cc, float m, float l, const float (&acc)[8]) {
  const float inv = l > 0.f ? 1.f / l : 0.f;
  float y[8];
#pragma unroll
  for (int e = 0; e < 8; ++e) y[e] = acc[e] * inv;
  store_chunk(o + cc * 8, y);
  if (cc == 0) *lse = l > 0.f ? m + __log2f(l) : INFINITY;
}

// 2^(e - 127) of an e8m0 byte as the f32 the scaled conversions take (they read its exponent field, so the
// zero byte is 2^-127: tests/test_mx_quant_oracle_gpu.py reads clamped blocks back through attn_decode)
__device__ __forceinline__ float e8m0_f32(unsigned e) { return __uint_as_float(e << 23); }

// MX8: kc / vc hold e4m3 bytes with one e8m0 scale per 32 elements.  A key row is 64 bytes, the lane's
// chunk 8 of them (inside one scale block: block c / 4); the gfx950 scaled conversions turn them into
// the packed bf16 of K (exact: 4 significant bits times a power of two) and the f32 of V, after which
// the sweep is the bf16 one.
//
// EXT (attn_extend): a wave's HW "heads" are rows (t, g) of a.P query positions t0 .. t0 + P - 1 and the G
// heads of the group, row index t' G + g, each with its own key limit n_t = clamp(lens[b] + t + extra);
// blockIdx.x carries (row tile, split).  The keys, slots, waves and both merges are attn_decode's for
// this G; the descriptors and the sweep end with the tile's largest limit, and a row's scores at and
// beyond its own limit are -inf: p = 0 there, so m, l and acc keep their bits (alpha = exp2(0) = 1, +0
// products of the finite rows the step itself appended), and row (t, g) ends with attn_decode's bits
// for extra + t.
template <int HW, bool MX8 = false, bool EXT = false>
__global__ __launch_bounds__(kDecThreads)
void attn_decode_kernel(const DecodeArgs a) {
  __shared__ alignas(16) float sh[kDecWaves][HW][kDecPart];
  const int split = EXT ? blockIdx.x % a.splits : blockIdx.x, j = blockIdx.y, b = blockIdx.z;
  const int t0 = EXT ? (blockIdx.x / a.splits) * a.P : 0;       // the block's first query position
  const int rows = EXT ? a.P * a.G : a.G;                       // rows (t, g) of the block
  const int lane = threadIdx.x & 63, slot = lane >> 3, c = lane & 7;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int parts = (rows + HW - 1) / HW;      // 1, or 2 for G > 8
  const int wpp = kDecWaves / parts;           // waves sweeping the range for one part's heads
  const int part = wave / wpp, wk = wave % wpp;
  const int g0 = part * HW;

  const int k0 = split * a.kps;
  // (EXT: of the block's last position, the largest limit)
  int n = a.lens[b] + a.extra + (EXT ? (t0 + a.P < a.T ? t0 + a.P : a.T) - 1 : 0);
  n = n < 0 ? 0 : (n > a.cap ? a.cap : n);
  const int k1 = k0 + a.kps < n ? k0 + a.kps : n;

  u32x4 qw[HW];
  int k1r[HW];                                 // EXT: the end of the range for row i (wave-uniform)
#pragma unroll
  for (int i = 0; i < HW; ++i) {
    qw[i] = u32x4{0u, 0u, 0u, 0u};
    k1r[i] = k1;
    if constexpr (EXT) {
      const int tt = t0 + (g0 + i) / a.G, g = (g0 + i) % a.G;
      k1r[i] = k0;                             // a row the block does not have: no key
      if (g0 + i < rows && tt < a.T) {
        qw[i] = load16<u32x4, kAligned16>(a.q + (long)b * a.qb + (long)tt * a.qt + (long)(j * a.G + g) * a.qh + c * 8);
        int nt = a.lens[b] + a.extra + tt;
        nt = nt < 0 ? 0 : (nt > a.cap ? a.cap : nt);
        k1r[i] = k0 + a.kps < nt ? k0 + a.kps : nt;
      }
    } else {
      if (g0 + i < a.G)
        qw[i] = load16<u32x4, kAligned16>(a.q + (long)b * a.qb + (long)(j * a.G + g0 + i) * a.qh + c * 8);
    }
  }

  // descriptors that end with row k1 - 1 of this (batch, key/value head): rows beyond read as zeros
  const bool any_key = k1 > k0;
  constexpr int ES = MX8 ? 1 : 2;              // bytes per cache element
  const long kbytes = any_key ? ((long)(k1 - 1) * a.ks + kDecD) * ES : 0;
  const long vbytes = any_key ? ((long)(k1 - 1) * a.vs + kDecD) * ES : 0;
  const __amdgpu_buffer_rsrc_t rk =
      make_rsrc(reinterpret_cast<const unsigned char*>(a.kc) + ((long)b * a.kb + (long)j * a.kh) * ES, kbytes);
  const __amdgpu_buffer_rsrc_t rv =
      make_rsrc(reinterpret_cast<const unsigned char*>(a.vc) + ((long)b * a.vb + (long)j * a.vh) * ES, vbytes);
  const int kstep = (int)a.ks * ES, vstep = (int)a.vs * ES;  // bytes per key (host: cap x stride fits an int)
  // the scales of the same rows, through descriptors that end with the same last row
  __amdgpu_buffer_rsrc_t rks = rk, rvs = rv;
  int ksstep = 0, vsstep = 0;
  if constexpr (MX8) {
    rks = make_rsrc(a.ksc + (long)b * a.ksb + (long)j * a.ksh, any_key ? (long)(k1 - 1) * a.kss + 2 : 0);
    rvs = make_rsrc(a.vsc + (long)b * a.vsb + (long)j * a.vsh, any_key ? (long)(k1 - 1) * a.vss + 2 : 0);
    ksstep = (int)a.kss;
    vsstep = (int)a.vss;
  }

  float m[HW], l[HW];
  f32x2 acc[HW][4];
#pragma unroll
  for (int i = 0; i < HW; ++i) {
    m[i] = -INFINITY;
    l[i] = 0.f;
#pragma unroll
    for (int e = 0; e < 4; ++e) acc[i][e] = f32x2{0.f, 0.f};
  }

  const int stride = wpp * kDecSlots;          // keys one step of this part's waves covers
  for (int base = k0; base < k1; base += stride * kDecUnroll) {
    int key[kDecUnroll];
    u32x4 kr[kDecUnroll];
    f32x2 vf[kDecUnroll][4];
    if constexpr (MX8) {
      u32x2 kq[kDecUnroll], vq[kDecUnroll];
      unsigned ke[kDecUnroll], ve[kDecUnroll];
#pragma unroll
      for (int u = 0; u < kDecUnroll; ++u) {
        key[u] = base + u * stride + wk * kDecSlots + slot;
        kq[u] = __builtin_amdgcn_raw_buffer_load_b64(rk, key[u] * kstep + c * 8, 0, 0);
        ke[u] = __builtin_amdgcn_raw_buffer_load_b8(rks, key[u] * ksstep + (c >> 2), 0, 0);
      }
#pragma unroll
      for (int u = 0; u < kDecUnroll; ++u) {
        vq[u] = __builtin_amdgcn_raw_buffer_load_b64(rv, key[u] * vstep + c * 8, 0, 0);
        ve[u] = __builtin_amdgcn_raw_buffer_load_b8(rvs, key[u] * vsstep + (c >> 2), 0, 0);
      }
#pragma unroll
      for (int u = 0; u < kDecUnroll; ++u) {
        const float ksf = e8m0_f32(ke[u]), vsf = e8m0_f32(ve[u]);
#pragma unroll
        for (int w = 0; w < 2; ++w) {          // (the half-word select is an immediate)
          kr[u][2 * w] = __builtin_bit_cast(unsigned, __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(kq[u][w], ksf, false));
          kr[u][2 * w + 1] = __builtin_bit_cast(unsigned, __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(kq[u][w], ksf, true));
          vf[u][2 * w] = __builtin_amdgcn_cvt_scalef32_pk_f32_fp8(vq[u][w], vsf, false);
          vf[u][2 * w + 1] = __builtin_amdgcn_cvt_scalef32_pk_f32_fp8(vq[u][w], vsf, true);
        }
      }
    } else {
      u32x4 vr[kDecUnroll];
#pragma unroll
      for (int u = 0; u < kDecUnroll; ++u) {
        key[u] = base + u * stride + wk * kDecSlots + slot;
        kr[u] = __builtin_amdgcn_raw_buffer_load_b128(rk, key[u] * kstep + c * 16, 0, 0);
      }
#pragma unroll
      for (int u = 0; u < kDecUnroll; ++u) vr[u] = __builtin_amdgcn_raw_buffer_load_b128(rv, key[u] * vstep + c * 16, 0, 0);
#pragma unroll
      for (int u = 0; u < kDecUnroll; ++u)
#pragma unroll
        for (int e = 0; e < 4; ++e) vf[u][e] = f32x2{bf16_lo(vr[u][e]), bf16_hi(vr[u][e])};
    }

#pragma unroll
    for (int i = 0; i < HW; ++i) {
      float s[kDecUnroll];
#pragma unroll
      for (int u = 0; u < kDecUnroll; ++u) {
        float d = 0.f;
#pragma unroll
        for (int w = 0; w < 4; ++w) d = dot2_bf16(kr[u][w], qw[i][w], d);
        d = sum8(d);
        s[u] = key[u] < (EXT ? k1r[i] : k1) ? d : -INFINITY;
      }
      float tmax = s[0];
#pragma unroll
      for (int u = 1; u < kDecUnroll; ++u) tmax = fmaxf(tmax, s[u]);
      // scores are compared raw (scale > 0 keeps the order); the scale is applied in the FMA below
      const float m_new = fmaxf(m[i], tmax * a.scale_log2);
      const float m_use = m_new == -INFINITY ? 0.f : m_new;
      const float alpha = dec_exp2(m[i] - m_use);
      float p[kDecUnroll], psum = 0.f;
#pragma unroll
      for (int u = 0; u < kDecUnroll; ++u) {
        p[u] = dec_exp2(s[u] * a.scale_log2 - m_use);
        psum += p[u];
      }
      l[i] = l[i] * alpha + psum;
      // no slot's running max moved (the usual case after the first keys): alpha is exactly 1
      if (__any(m_new != m[i])) {
        const f32x2 al2 = {alpha, alpha};
#pragma unroll
        for (int e = 0; e < 4; ++e) acc[i][e] = acc[i][e] * al2;
      }
      m[i] = m_new;
#pragma unroll
      for (int u = 0; u < kDecUnroll; ++u) {
        const float pb = bf2f(f2bf(p[u]));     // probabilities rounded to bf16 before P.V
        const f32x2 pb2 = {pb, pb};
#pragma unroll
        for (int e = 0; e < 4; ++e) acc[i][e] = pb2 * vf[u][e] + acc[i][e];
      }
    }
  }

  // the 8 slots of the wave, merged into slot 0 (lanes 0..7) in a fixed order
#pragma unroll
  for (int i = 0; i < HW; ++i) {
    float av[8];
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      av[2 * e] = acc[i][e][0];
      av[2 * e + 1] = acc[i][e][1];
    }
#pragma unroll
    for (int x = kDecChunks; x < 64; x <<= 1) {
      const float m2 = __shfl_xor(m[i], x, 64), l2 = __shfl_xor(l[i], x, 64);
      float a2[8];
#pragma unroll
      for (int e = 0; e < 8; ++e) a2[e] = __shfl_xor(av[e], x, 64);
      dec_merge(m[i], l[i], av, m2, l2, a2);
    }
    if (slot == 0) {
      store_chunk(&sh[wave][i][c * 8], av);
      store_chunk(&sh[wave][i][c * 8 + 4], av + 4);
      if (c == 0) {
        sh[wave][i][kDecD] = m[i];
        sh[wave][i][kDecD + 1] = l[i];
      }
    }
  }
  __syncthreads();

  // the waves of a head's part, in ascending order: thread (g, chunk)
  const int t = threadIdx.x;
  if (t < rows * kDecChunks) {
    const int r = t >> 3, cc = t & 7, pg = r / HW, gi = r % HW;
    float mm = -INFINITY, ll = 0.f, av[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    for (int w = pg * wpp; w < (pg + 1) * wpp; ++w) {
      float a2[8];
      load_chunk(&sh[w][gi][cc * 8], a2);
      load_chunk(&sh[w][gi][cc * 8 + 4], a2 + 4);
      dec_merge(mm, ll, av, sh[w][gi][kDecD], sh[w][gi][kDecD + 1], a2);
    }
    const int tt = EXT ? t0 + r / a.G : 0, h = j * a.G + (EXT ? r % a.G : r);
    if (EXT && tt >= a.T) return;              // a position past the last tile's end
    const long bt = EXT ? (long)b * a.T + tt : b;
    if (a.splits == 1) {
      dec_store_out(a.o + (long)b * a.ob + (EXT ? (long)tt * a.ot : 0L) + (long)h * a.oh, a.lse + bt * a.H + h, cc, mm,
                    ll, av);
    } else {
      float* p = a.ws + ((bt * a.H + h) * a.splits + split) * kDecPart;
      store_chunk(p + cc * 8, av);
      store_chunk(p + cc * 8 + 4, av + 4);
      if (cc == 0) {
        p[kDecD] = mm;
        p[kDecD + 1] = ll;
      }
    }
  }
}

// The partials of one (b, t, h) per wave (T = 1 for attn_decode): lane = (slot, chunk).  Pass 1 finds the largest m of all splits
// (exact, whatever the order).  Pass 2: slot j adds the splits j, j + 8, .. in ascending order, each
// weighted by exp2(m_s - M), with the loads of 4 splits in flight; the 8 slots are then added by a
// fixed tree of plain adds.  Every order is fixed, so the bits are the same on every run.
constexpr int kMergeUnroll = 4;
__global__ __launch_bounds__(64)
void decode_merge_kernel(const DecodeArgs a) {
  const int lane = threadIdx.x, slot = lane >> 3, cc = lane & 7;
  const long bh = blockIdx.x;
  const float* base = a.ws + bh * a.splits * kDecPart;
  float mx = -INFINITY;
  for (int s = lane; s < a.splits; s += 64) mx = fmaxf(mx, base[(long)s * kDecPart + kDecD]);
  mx = warp_max64(mx);
  const float mu = mx == -INFINITY ? 0.f : mx;
  float ll = 0.f, av[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  for (int s0 = slot; s0 < a.splits; s0 += kDecSlots * kMergeUnroll) {
    float a2[kMergeUnroll][8], m2[kMergeUnroll], l2[kMergeUnroll];
#pragma unroll
    for (int u = 0; u < kMergeUnroll; ++u) {
      const int s = s0 + u * kDecSlots;
      const float* p = base + (long)s * kDecPart;
      m2[u] = -INFINITY;
      l2[u] = 0.f;
#pragma unroll
      for (int e = 0; e < 8; ++e) a2[u][e] = 0.f;
      if (s < a.splits) {                         // (uniform over a slot's 8 lanes)
        load_chunk(p + cc * 8, a2[u]);
        load_chunk(p + cc * 8 + 4, a2[u] + 4);
        m2[u] = p[kDecD];
        l2[u] = p[kDecD + 1];
      }
    }
#pragma unroll
    for (int u = 0; u < kMergeUnroll; ++u) {
      const float w = dec_exp2(m2[u] - mu);       // 0 for an empty partial and past the last split
      ll += l2[u] * w;
#pragma unroll
      for (int e = 0; e < 8; ++e) av[e] += a2[u][e] * w;
    }
  }
#pragma unroll
  for (int x = kDecChunks; x < 64; x <<= 1) {
    ll += __shfl_xor(ll, x, 64);
#pragma unroll
    for (int e = 0; e < 8; ++e) av[e] += __shfl_xor(av[e], x, 64);
  }
  if (slot == 0) {
    const long bt = bh / a.H, h = bh % a.H;
    dec_store_out(a.o + (bt / a.T) * a.ob + (bt % a.T) * a.ot + h * a.oh, a.lse + bh, cc, mx, ll, av);
  }
}

// ---- the plan: pure, of the capacity and never of the lengths
inline void plan_decode(int B, int Hkv, int cap, int cus, int* splits, int* kps) {
  const long tiles = ((long)cap + kDecKeyTile - 1) / kDecKeyTile;
  const long groups = (long)B * Hkv;
  long s = 1;
  if (tiles > kDecOneSplitTiles) {
    const long want = ((long)kDecBlocksPerCu * cus + groups - 1) / groups;   // several blocks per CU
    const long fill = ((long)cus + groups - 1) / groups;                      // one block per CU
    const long most = (tiles + kDecMinTiles - 1) / kDecMinTiles;              // a split is worth a block
    s = want < most ? want : most;
    if (s < fill) {                      // too few blocks for the chip: allow splits of half the size
      const long most2 = (tiles + kDecMinTiles / 2 - 1) / (kDecMinTiles / 2);
      s = fill < most2 ? fill : most2;
    }
  }
  const long per = (tiles + s - 1) / s;
  *kps = (int)(per * kDecKeyTile);
  *splits = (int)((tiles + per - 1) / per);
}

inline int decode_launch_plan(int B, int Hkv, int cap, int* splits, int* kps) {
  if (g_dec_splits > 0) {
    if (g_dec_keys % kDecKeyTile != 0 || (long)g_dec_splits * g_dec_keys < cap) return (int)hipErrorInvalidValue;
    *splits = g_dec_splits;
    *kps = g_dec_keys;
    return 0;
  }
  plan_decode(B, Hkv, cap, ljs_device_cus(), splits, kps);
  return 0;
}

inline bool dec_aligned(const void* p, const long* st) {
  return p && st && (((uintptr_t)p) & 15u) == 0 && st[0] % 8 == 0 && st[1] % 8 == 0 && st[2] % 8 == 0;
}

// ---- kv_append
struct AppTensor {
  const bf16_t* in;
  bf16_t* out;
  long ib, it, ih;            // input strides (elements): batch, position, head
  long ob, op, oh;            // output strides
  long first;                 // its first work item
  int H, rotate, cache;
};

struct AppendArgs {
  AppTensor t[3];             // k -> kc, v -> vc, q -> q_out
  const float *cos_t, *sin_t;
  const int* lens;
  long total;
  int nt, T, cap;
};

__global__ __launch_bounds__(kRowBlockThreads)
void kv_append_kernel(const AppendArgs a) {
  constexpr int h = kDecD / 2;
  const long step = (long)gridDim.x * kRowBlockThreads;
  for (long item = (long)blockIdx.x * kRowBlockThreads + threadIdx.x; item < a.total; item += step) {
    int which = 0;
    if (a.nt > 1 && item >= a.t[1].first) which = 1;
    if (a.nt > 2 && item >= a.t[2].first) which = 2;
    const AppTensor& x = a.t[which];
    long r = item - x.first;
    const int jj = (int)(r % 4);
    r /= 4;
    const int hd = (int)(r % x.H);
    r /= x.H;
    const int tt = (int)(r % a.T);
    const long b = r / a.T;
    const long p = (a.lens ? (long)a.lens[b] : 0L) + tt;
    const bool inside = p >= 0 && p < a.cap;
    if (x.cache && !inside) continue;             // no store outside the cache
    bf16_t* dst = x.out + b * x.ob + (x.cache ? p : (long)tt) * x.op + (long)hd * x.oh + jj * 8;
    if (!inside) {                                // q_out of a sequence that is full: zeros
      const u32x4 z = {0u, 0u, 0u, 0u};
      store16<kAligned16>(dst, z);
      store16<kAligned16>(dst + h, z);
      continue;
    }
    const bf16_t* src = x.in + b * x.ib + (long)tt * x.it + (long)hd * x.ih + jj * 8;
    if (!x.rotate) {
      const u32x4 lo = load16<u32x4, kAligned16>(src), hi = load16<u32x4, kAligned16>(src + h);
      store16<kAligned16>(dst, lo);
      store16<kAligned16>(dst + h, hi);
      continue;
    }
    const long trow = p * (long)h + jj * 8;
    float x0[8], x1[8], c[8], sn[8], y0[8], y1[8];
    load_chunk8(src, x0);
    load_chunk8(src + h, x1);
    load_chunk8(a.cos_t + trow, c);
    load_chunk8(a.sin_t + trow, sn);
#pragma unroll
    for (int e = 0; e < 8; ++e) {                 // rope_kernel's expressions
      const float sg = sn[e];
      y0[e] = x0[e] * c[e] - x1[e] * sg;
      y1[e] = x1[e] * c[e] + x0[e] * sg;
    }
    store_chunk8(dst, y0);
    store_chunk8(dst + h, y1);
  }
}

// ---- kv_append into an MX-fp8 cache
// The bf16 kernel's work items and position rule; a cached row is stored as quantize_mx_ref of the bf16
// row the bf16 cache would hold: 64 e4m3 bytes and two e8m0 scale bytes (elements 0..31, 32..63).  The
// four items of a row are the four lanes of a quad (item % 4 is the lane's, as the tensors' first
// items, the total and the grid stride are all multiples of 4), and the quad takes every branch
// together, so a block maximum is an integer max of bf16 magnitude bits over the lane's 8 elements and
// then over the quad by two DPP quad_perm steps.  No LDS, no atomics, no workspace.
struct AppendQ8Args {
  AppendArgs a;               // t[0].out / t[1].out: the e4m3 bytes, their o* strides in bytes
  unsigned char* sc[2];       // the scales of k and v, (B, cap, Hkv, 2)
  long sb[2], sp[2], sh[2];   // their (batch, position, head) strides in bytes
};

__device__ __forceinline__ unsigned quad_max(unsigned v) {
  v = max(v, (unsigned)__builtin_amdgcn_update_dpp(0, (int)v, 0xB1, 0xf, 0xf, false));   // quad_perm [1,0,3,2]
  return max(v, (unsigned)__builtin_amdgcn_update_dpp(0, (int)v, 0x4E, 0xf, 0xf, false));   // quad_perm [2,3,0,1]
}

// the largest bf16 magnitude (bits) of four packed pairs
__device__ __forceinline__ unsigned amax_bits8(const u32x4& w) {
  unsigned mx = 0u;
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    const unsigned m = w[e] & 0x7fff7fffu;
    mx = max(mx, max(m & 0xffffu, m >> 16));
  }
  return mx;
}

__global__ __launch_bounds__(kRowBlockThreads)
void kv_append_q8_kernel(const AppendQ8Args qa) {
  constexpr int h = kDecD / 2;
  const AppendArgs& a = qa.a;
  const long step = (long)gridDim.x * kRowBlockThreads;
  for (long item = (long)blockIdx.x * kRowBlockThreads + threadIdx.x; item < a.total; item += step) {
    int which = 0;
    if (item >= a.t[1].first) which = 1;
    if (a.nt > 2 && item >= a.t[2].first) which = 2;
    const AppTensor& x = a.t[which];
    long r = item - x.first;
    const int jj = (int)(r % 4);
    r /= 4;
    const int hd = (int)(r % x.H);
    r /= x.H;
    const int tt = (int)(r % a.T);
    const long b = r / a.T;
    const long p = (a.lens ? (long)a.lens[b] : 0L) + tt;
    const bool inside = p >= 0 && p < a.cap;
    if (x.cache && !inside) continue;             // no store outside the cache: neither bytes nor scales
    if (!x.cache && !inside) {                    // q_out of a sequence that is full: zeros
      bf16_t* dst = x.out + b * x.ob + (long)tt * x.op + (long)hd * x.oh + jj * 8;
      const u32x4 z = {0u, 0u, 0u, 0u};
      store16<kAligned16>(dst, z);
      store16<kAligned16>(dst + h, z);
      continue;
    }
    const bf16_t* src = x.in + b * x.ib + (long)tt * x.it + (long)hd * x.ih + jj * 8;
    u32x4 lo, hi;                                 // the row's chunks jj and jj + 4 as the bf16 cache holds them
    if (!x.rotate) {
      lo = load16<u32x4, kAligned16>(src);
      hi = load16<u32x4, kAligned16>(src + h);
    } else {
      const long trow = p * (long)h + jj * 8;
      float x0[8], x1[8], c[8], sn[8], y0[8], y1[8];
      load_chunk8(src, x0);
      load_chunk8(src + h, x1);
      load_chunk8(a.cos_t + trow, c);
      load_chunk8(a.sin_t + trow, sn);
#pragma unroll
      for (int e = 0; e < 8; ++e) {               // rope_kernel's expressions
        const float sg = sn[e];
        y0[e] = x0[e] * c[e] - x1[e] * sg;
        y1[e] = x1[e] * c[e] + x0[e] * sg;
      }
      lo = pack_bf16x8(y0);                       // rope's bits first, then the quantiser
      hi = pack_bf16x8(y1);
    }
    if (!x.cache) {
      bf16_t* dst = x.out + b * x.ob + (long)tt * x.op + (long)hd * x.oh + jj * 8;
      store16<kAligned16>(dst, lo);
      store16<kAligned16>(dst + h, hi);
      continue;
    }
    const int e0 = mx_exponent(__uint_as_float(quad_max(amax_bits8(lo)) << 16));
    const int e1 = mx_exponent(__uint_as_float(quad_max(amax_bits8(hi)) << 16));
    const float s0 = mx_scale_pow2(e0), s1 = mx_scale_pow2(e1);
    unsigned char* dst = reinterpret_cast<unsigned char*>(x.out) + b * x.ob + p * x.op + (long)hd * x.oh + jj * 8;
    *reinterpret_cast<u32x2*>(dst) = u32x2{cvt4_e4m3_bf16(lo[0], lo[1], s0), cvt4_e4m3_bf16(lo[2], lo[3], s0)};
    *reinterpret_cast<u32x2*>(dst + h) = u32x2{cvt4_e4m3_bf16(hi[0], hi[1], s1), cvt4_e4m3_bf16(hi[2], hi[3], s1)};
    if (jj == 0)
      *reinterpret_cast<unsigned short*>(qa.sc[which] + b * qa.sb[which] + p * qa.sp[which] + (long)hd * qa.sh[which]) =
          (unsigned short)((e0 + 127) | ((e1 + 127) << 8));
  }
}

__global__ void lens_add_kernel(int* lens, int B, int n) {
  for (int i = threadIdx.x; i < B; i += blockDim.x) lens[i] += n;
}

}  // namespace

// tests: force `n` splits of `keys` keys (keys a multiple of the key tile, n x keys >= cap, else the
// launcher returns hipErrorInvalidValue); n <= 0 restores the plan
LJS_API int ljs_decode_set_splits(int n, int keys) {
  g_dec_splits = n > 0 ? n : 0;
  g_dec_keys = n > 0 ? keys : 0;
  return 0;
}

LJS_API int ljs_decode_key_tile() { return kDecKeyTile; }
LJS_API int ljs_decode_part_floats() { return kDecPart; }
LJS_API int ljs_decode_max_group() { return kDecMaxG; }

// out[0] = splits, out[1] = keys_per_split of (B, Hkv, cap) on a device of `cus` compute units: pure
LJS_API int ljs_decode_plan(int B, int Hkv, int cap, int cus, int* out) {
  if (B < 1 || Hkv < 1 || cap < 1 || cus < 1 || !out) return (int)hipErrorInvalidValue;
  plan_decode(B, Hkv, cap, cus, out, out + 1);
  return 0;
}

// the plan the next ljs_attn_decode of this shape launches (the forced one, or the pure plan for this
// device): what the workspace is sized from
LJS_API int ljs_decode_launch_plan(int B, int Hkv, int cap, int* out) {
  if (B < 1 || Hkv < 1 || cap < 1 || !out) return (int)hipErrorInvalidValue;
  return decode_launch_plan(B, Hkv, cap, out, out + 1);
}

namespace {

// an MX-fp8 cache operand: e4m3 bytes (B, cap, Hkv, 64), 16-byte aligned base and byte strides; its e8m0
// scales (B, cap, Hkv, 2): a 2-byte aligned base and even byte strides (one lane stores both bytes)
inline bool q8_aligned(const void* p, const long* st) {
  return p && st && (((uintptr_t)p) & 15u) == 0 && st[0] % 16 == 0 && st[1] % 16 == 0 && st[2] % 16 == 0;
}
inline bool q8_scale_aligned(const void* p, const long* st) {
  return p && st && (((uintptr_t)p) & 1u) == 0 && st[0] % 2 == 0 && st[1] % 2 == 0 && st[2] % 2 == 0;
}

// the checks and the work items the two append launchers share (the cache operands' own alignment is
// the caller's): 0 and *a filled, or hipErrorInvalidValue
inline int append_plan(const void* k, const void* v, const void* q, void* kc, void* vc, void* q_out, int B, int T,
                       int H, int Hkv, int cap, const long* sk, const long* sv, const long* sq, const long* skc,
                       const long* svc, const long* sqo, const void* lens, const void* cos_t, const void* sin_t,
                       long table_rows, AppendArgs* out) {
  const bool rot = cos_t != nullptr;
  if (B < 1 || T < 1 || Hkv < 1 || cap < 1 || (cos_t == nullptr) != (sin_t == nullptr) ||
      (q == nullptr) != (q_out == nullptr) || (q && (!rot || H < 1)))
    return (int)hipErrorInvalidValue;
  if (rot && (table_rows < cap || (((uintptr_t)cos_t) & 15u) || (((uintptr_t)sin_t) & 15u)))
    return (int)hipErrorInvalidValue;
  if (lens && (((uintptr_t)lens) & 3u)) return (int)hipErrorInvalidValue;
  if (!dec_aligned(k, sk) || !dec_aligned(v, sv) || (q && (!dec_aligned(q, sq) || !dec_aligned(q_out, sqo))))
    return (int)hipErrorInvalidValue;
  AppendArgs a{};
  const long per_kv = (long)B * T * Hkv * 4;
  a.t[0] = AppTensor{(const bf16_t*)k, (bf16_t*)kc, sk[0], sk[1], sk[2], skc[0], skc[1], skc[2], 0, Hkv, rot, 1};
  a.t[1] = AppTensor{(const bf16_t*)v, (bf16_t*)vc, sv[0], sv[1], sv[2], svc[0], svc[1], svc[2], per_kv, Hkv, 0, 1};
  a.nt = 2;
  a.total = 2 * per_kv;
  if (q) {
    a.t[2] = AppTensor{(const bf16_t*)q, (bf16_t*)q_out, sq[0], sq[1], sq[2], sqo[0], sqo[1], sqo[2], a.total, H, 1, 0};
    a.nt = 3;
    a.total += (long)B * T * H * 4;
  }
  a.cos_t = (const float*)cos_t;
  a.sin_t = (const float*)sin_t;
  a.lens = (const int*)lens;
  a.T = T;
  a.cap = cap;
  *out = a;
  return 0;
}

inline dim3 append_grid(const AppendArgs& a) {
  const long need = (a.total + kRowBlockThreads - 1) / kRowBlockThreads;
  const long most = (long)ljs_device_cus() * kAppBlocksPerCu;
  return dim3((unsigned)(need < most ? need : most));
}

}  // namespace

// k, v (B, T, Hkv, 64) -> kc, vc (B, cap, Hkv, 64) at rows base[b] + t, base = lens (int32 [B], device)
// or 0 when lens is null; q (B, T, H, 64) -> q_out (B, T, H, 64) when both are given.  cos_t / sin_t (f32
// [table_rows][32], table_rows >= cap) rotate k and q; both null: k is copied as it is.  s*: the
// (batch, position, head) strides in elements.  Returns hipErrorInvalidValue, and launches and records
// nothing, for an empty shape, a misaligned base or stride, one of q / q_out alone, q without a
// table, or a table shorter than the cache.
LJS_API int ljs_kv_append(const void* k, const void* v, const void* q, void* kc, void* vc, void* q_out, int B, int T,
                          int H, int Hkv, int cap, const long* sk, const long* sv, const long* sq, const long* skc,
                          const long* svc, const long* sqo, const void* lens, const void* cos_t, const void* sin_t,
                          long table_rows, hipStream_t st) {
  if (!dec_aligned(kc, skc) || !dec_aligned(vc, svc)) return (int)hipErrorInvalidValue;
  AppendArgs a{};
  if (append_plan(k, v, q, kc, vc, q_out, B, T, H, Hkv, cap, sk, sv, sq, skc, svc, sqo, lens, cos_t, sin_t, table_rows,
                  &a) != 0)
    return (int)hipErrorInvalidValue;
  const dim3 grid = append_grid(a);
  hipLaunchKernelGGL(kv_append_kernel, grid, dim3(kRowBlockThreads), 0, st, a);
  ljs_launch_rec(q ? "kv_append<rot,q>" : (cos_t ? "kv_append<rot>" : "kv_append<copy>"), grid, kRowBlockThreads);
  return (int)hipGetLastError();
}

// ljs_kv_append into an MX-fp8 cache: kc / vc are e4m3 bytes (B, cap, Hkv, 64) and kcs / vcs their e8m0
// scales (B, cap, Hkv, 2) -- of every row written, quantize_mx_ref of the bf16 row ljs_kv_append would
// have stored; q_out stays bf16.  skc / svc / skcs / svcs: (batch, position, head) strides in bytes.
// Refuses what ljs_kv_append refuses, and a null or odd scale base, an odd scale stride, or a cache
// base or stride that is not a multiple of 16 bytes.
LJS_API int ljs_kv_append_q8(const void* k, const void* v, const void* q, void* kc, void* vc, void* kcs, void* vcs,
                             void* q_out, int B, int T, int H, int Hkv, int cap, const long* sk, const long* sv,
                             const long* sq, const long* skc, const long* svc, const long* skcs, const long* svcs,
                             const long* sqo, const void* lens, const void* cos_t, const void* sin_t, long table_rows,
                             hipStream_t st) {
  if (!q8_aligned(kc, skc) || !q8_aligned(vc, svc) || !q8_scale_aligned(kcs, skcs) || !q8_scale_aligned(vcs, svcs))
    return (int)hipErrorInvalidValue;
  AppendQ8Args qa{};
  if (append_plan(k, v, q, kc, vc, q_out, B, T, H, Hkv, cap, sk, sv, sq, skc, svc, sqo, lens, cos_t, sin_t, table_rows,
                  &qa.a) != 0)
    return (int)hipErrorInvalidValue;
  qa.sc[0] = (unsigned char*)kcs;
  qa.sc[1] = (unsigned char*)vcs;
  qa.sb[0] = skcs[0]; qa.sp[0] = skcs[1]; qa.sh[0] = skcs[2];
  qa.sb[1] = svcs[0]; qa.sp[1] = svcs[1]; qa.sh[1] = svcs[2];
  const dim3 grid = append_grid(qa.a);
  hipLaunchKernelGGL(kv_append_q8_kernel, grid, dim3(kRowBlockThreads), 0, st, qa);
  ljs_launch_rec(q ? "kv_append<rot,q,mx8>" : (cos_t ? "kv_append<rot,mx8>" : "kv_append<copy,mx8>"), grid,
                 kRowBlockThreads);
  return (int)hipGetLastError();
}

namespace {

// attn_extend's instance for T > 1 positions of groups of G heads: the positions P one block carries (8 / G
// of them for G <= 8, G rounded up to attn_decode's instance; no more than T rounded up to a power of two,
// which gives the same row tiles with fewer idle rows), the rows HW of a wave and the logged name
struct ExtInstance {
  int P, HW;
  const char* name;
};
inline ExtInstance extend_instance(int G, int T, bool mx8) {
  static const char* const names[2][8] = {
      {"attn_extend<G1,P2>", "attn_extend<G1,P4>", "attn_extend<G1,P8>", "attn_extend<G2,P2>", "attn_extend<G2,P4>",
       "attn_extend<G4,P2>", "attn_extend<G8,P1>", "attn_extend<G16,P1>"},
      {"attn_extend<G1,P2,mx8>", "attn_extend<G1,P4,mx8>", "attn_extend<G1,P8,mx8>", "attn_extend<G2,P2,mx8>",
       "attn_extend<G2,P4,mx8>", "attn_extend<G4,P2,mx8>", "attn_extend<G8,P1,mx8>", "attn_extend<G16,P1,mx8>"}};
  const int t2 = T <= 2 ? 2 : (T <= 4 ? 4 : 8);
  if (G == 1) return {t2, t2, names[mx8][t2 == 2 ? 0 : (t2 == 4 ? 1 : 2)]};
  if (G == 2) return t2 == 2 ? ExtInstance{2, 4, names[mx8][3]} : ExtInstance{4, 8, names[mx8][4]};
  if (G <= 4) return {2, 8, names[mx8][5]};
  return {1, 8, names[mx8][G <= 8 ? 6 : 7]};
}

// the launch the decode and extend entries share: T = 1 is attn_decode, T > 1 attn_extend over the keys
// [0, lens[b] + extra + t); ES: bytes per cache element; kcs / vcs: the scales (MX8 only)
template <bool MX8>
int decode_launch(const void* q, const void* kc, const void* vc, const void* kcs, const void* vcs, void* o, void* lse,
                  void* ws, long ws_floats, const void* lens, int B, int T, int H, int Hkv, int cap, const long* sq,
                  const long* skc, const long* svc, const long* skcs, const long* svcs, const long* so, float scale,
                  int extra, hipStream_t st) {
  constexpr long ES = MX8 ? 1 : 2;
  if (T < 1 || T > kExtMaxT) return (int)hipErrorInvalidValue;
  if (B < 1 || H < 1 || Hkv < 1 || cap < 1 || H % Hkv != 0 || H / Hkv > kDecMaxG || !(scale > 0.f) || extra < 0 ||
      B > 65535 || Hkv > 65535 || (long)B * T * H > 0x7fffffffL || !lens || !lse || (((uintptr_t)lens) & 3u) || (((uintptr_t)lse) & 3u))
    return (int)hipErrorInvalidValue;
  if (!dec_aligned(q, sq) || !dec_aligned(o, so)) return (int)hipErrorInvalidValue;
  if (MX8 ? (!q8_aligned(kc, skc) || !q8_aligned(vc, svc) || !q8_scale_aligned(kcs, skcs) || !q8_scale_aligned(vcs, svcs))
          : (!dec_aligned(kc, skc) || !dec_aligned(vc, svc)))
    return (int)hipErrorInvalidValue;
  // a load's byte offset (of up to one unrolled block step past the cache) stays a positive int
  const long reach = (long)cap + kDecKeyTile * kDecUnroll;
  if (skc[1] < kDecD || svc[1] < kDecD || reach * skc[1] * ES >= 0x7fffffffL || reach * svc[1] * ES >= 0x7fffffffL)
    return (int)hipErrorInvalidValue;
  if (MX8 && (skcs[1] < 2 || svcs[1] < 2 || reach * skcs[1] >= 0x7fffffffL || reach * svcs[1] >= 0x7fffffffL))
    return (int)hipErrorInvalidValue;
  DecodeArgs a{};
  if (decode_launch_plan(B, Hkv, cap, &a.splits, &a.kps) != 0) return (int)hipErrorInvalidValue;
  if (a.splits > 1 && (!ws || (((uintptr_t)ws) & 15u) || ws_floats < (long)B * T * H * a.splits * kDecPart))
    return (int)hipErrorInvalidValue;
  a.q = (const bf16_t*)q;
  a.kc = (const bf16_t*)kc;
  a.vc = (const bf16_t*)vc;
  a.o = (bf16_t*)o;
  a.lse = (float*)lse;
  a.ws = (float*)ws;
  a.lens = (const int*)lens;
  a.qb = sq[0]; a.qt = sq[1]; a.qh = sq[2];
  a.kb = skc[0]; a.ks = skc[1]; a.kh = skc[2];
  a.vb = svc[0]; a.vs = svc[1]; a.vh = svc[2];
  a.ob = so[0]; a.ot = so[1]; a.oh = so[2];
  a.T = T; a.P = 1;
  a.B = B; a.H = H; a.Hkv = Hkv; a.G = H / Hkv; a.cap = cap; a.extra = extra;
  a.scale_log2 = scale * 1.4426950408889634f;
  if (MX8) {
    a.ksc = (const unsigned char*)kcs;
    a.vsc = (const unsigned char*)vcs;
    a.ksb = skcs[0]; a.kss = skcs[1]; a.ksh = skcs[2];
    a.vsb = svcs[0]; a.vss = svcs[1]; a.vsh = svcs[2];
  }
  dim3 grid((unsigned)a.splits, (unsigned)Hkv, (unsigned)B);
  const char* name;
  if (T > 1) {
    const ExtInstance x = extend_instance(a.G, T, MX8);
    a.P = x.P;
    grid.x = (unsigned)(a.splits * ((T + x.P - 1) / x.P));      // (row tile, split)
    name = x.name;
    if (x.HW == 2)
      hipLaunchKernelGGL((attn_decode_kernel<2, MX8, true>), grid, dim3(kDecThreads), 0, st, a);
    else if (x.HW == 4)
      hipLaunchKernelGGL((attn_decode_kernel<4, MX8, true>), grid, dim3(kDecThreads), 0, st, a);
    else
      hipLaunchKernelGGL((attn_decode_kernel<8, MX8, true>), grid, dim3(kDecThreads), 0, st, a);
  } else if (a.G == 1) {
    hipLaunchKernelGGL((attn_decode_kernel<1, MX8>), grid, dim3(kDecThreads), 0, st, a);
    name = MX8 ? "attn_decode<G1,mx8>" : "attn_decode<G1>";
  } else if (a.G == 2) {
    hipLaunchKernelGGL((attn_decode_kernel<2, MX8>), grid, dim3(kDecThreads), 0, st, a);
    name = MX8 ? "attn_decode<G2,mx8>" : "attn_decode<G2>";
  } else if (a.G <= 4) {
    hipLaunchKernelGGL((attn_decode_kernel<4, MX8>), grid, dim3(kDecThreads), 0, st, a);
    name = MX8 ? "attn_decode<G4,mx8>" : "attn_decode<G4>";
  } else if (a.G <= 8) {
    hipLaunchKernelGGL((attn_decode_kernel<8, MX8>), grid, dim3(kDecThreads), 0, st, a);
    name = MX8 ? "attn_decode<G8,mx8>" : "attn_decode<G8>";
  } else {
    hipLaunchKernelGGL((attn_decode_kernel<8, MX8>), grid, dim3(kDecThreads), 0, st, a);
    name = MX8 ? "attn_decode<G16,mx8>" : "attn_decode<G16>";
  }
  ljs_launch_rec(name, grid, kDecThreads);
  int rc = (int)hipGetLastError();
  if (rc != 0 || a.splits == 1) return rc;
  const dim3 mgrid((unsigned)(B * T * H));
  hipLaunchKernelGGL(decode_merge_kernel, mgrid, dim3(64), 0, st, a);
  ljs_launch_rec("decode_merge", mgrid, 64);
  return (int)hipGetLastError();
}

}  // namespace

// q (B, 1, H, 64), kc / vc (B, cap, Hkv, 64) -> o (B, 1, H, 64) bf16, lse (B, H) f32 over the keys [0,
// min(lens[b] + extra, cap)) (the head of the file).  ws: f32 workspace of ws_floats floats, at least B H
// splits kDecPart of them when the plan has more than one split.  s*: (batch, position, head) strides in
// elements.  Returns hipErrorInvalidValue, and launches and records nothing, for an empty shape, H %
// Hkv != 0, H / Hkv > 16, scale <= 0, extra < 0, a misaligned base or stride, a key stride below 64, a
// cache whose byte offsets do not fit 31 bits, an invalid forced plan or a workspace that is too small.
LJS_API int ljs_attn_decode(const void* q, const void* kc, const void* vc, void* o, void* lse, void* ws, long ws_floats,
                            const void* lens, int B, int H, int Hkv, int cap, const long* sq, const long* skc,
                            const long* svc, const long* so, float scale, int extra, hipStream_t st) {
  return decode_launch<false>(q, kc, vc, nullptr, nullptr, o, lse, ws, ws_floats, lens, B, 1, H, Hkv, cap, sq, skc, svc,
                              nullptr, nullptr, so, scale, extra, st);
}

// ljs_attn_decode over an MX-fp8 cache: kc / vc e4m3 bytes (B, cap, Hkv, 64), kcs / vcs their e8m0 scales
// (B, cap, Hkv, 2), all four with (batch, position, head) strides in bytes; q, o, lse, ws, the plan and
// the merge launch as there.  The same refusals, with the 31-bit offset check on 1-byte elements and
// on the scales, plus: a null or odd scale base, an odd scale stride, a scale row stride below 2, a
// cache base or stride that is not a multiple of 16 bytes.
LJS_API int ljs_attn_decode_q8(const void* q, const void* kc, const void* vc, const void* kcs, const void* vcs, void* o,
                               void* lse, void* ws, long ws_floats, const void* lens, int B, int H, int Hkv, int cap,
                               const long* sq, const long* skc, const long* svc, const long* skcs, const long* svcs,
                               const long* so, float scale, int extra, hipStream_t st) {
  return decode_launch<true>(q, kc, vc, kcs, vcs, o, lse, ws, ws_floats, lens, B, 1, H, Hkv, cap, sq, skc, svc, skcs,
                             svcs, so, scale, extra, st);
}

LJS_API int ljs_extend_max_positions() { return kExtMaxT; }

// q (B, T, H, 64) -> o (B, T, H, 64) bf16, lse (B, T, H) f32: row (b, t, h) over the keys [0, clamp(lens[b] + t + 1,
// 0, cap)), after an append of the T positions that lens does not count yet -- the bits ljs_attn_decode
// writes for (b, h) with extra = t + 1 under the same plan.  T == 1 IS that call (its launches, its
// records).  ws: at least B T H splits kDecPart floats when the plan has more than one split.  Refuses
// what ljs_attn_decode refuses, and T outside [1, 64].
LJS_API int ljs_attn_extend(const void* q, const void* kc, const void* vc, void* o, void* lse, void* ws, long ws_floats,
                            const void* lens, int B, int T, int H, int Hkv, int cap, const long* sq, const long* skc,
                            const long* svc, const long* so, float scale, hipStream_t st) {
  return decode_launch<false>(q, kc, vc, nullptr, nullptr, o, lse, ws, ws_floats, lens, B, T, H, Hkv, cap, sq, skc, svc,
                              nullptr, nullptr, so, scale, 1, st);
}

// ljs_attn_extend over an MX-fp8 cache (ljs_attn_decode_q8's operands and refusals)
LJS_API int ljs_attn_extend_q8(const void* q, const void* kc, const void* vc, const void* kcs, const void* vcs, void* o,
                               void* lse, void* ws, long ws_floats, const void* lens, int B, int T, int H, int Hkv,
                               int cap, const long* sq, const long* skc, const long* svc, const long* skcs,
                               const long* svcs, const long* so, float scale, hipStream_t st) {
  return decode_launch<true>(q, kc, vc, kcs, vcs, o, lse, ws, ws_floats, lens, B, T, H, Hkv, cap, sq, skc, svc, skcs,
                             svcs, so, scale, 1, st);
}

// lens[0 .. B) += n: one small launch after the last layer of a decode step
LJS_API int ljs_lens_add(void* lens, int B, int n, hipStream_t st) {
  if (!lens || B < 1 || (((uintptr_t)lens) & 3u)) return (int)hipErrorInvalidValue;
  hipLaunchKernelGGL(lens_add_kernel, dim3(1), dim3(64), 0, st, (int*)lens, B, n);
  ljs_launch_rec("lens_add", dim3(1), 64);
  return (int)hipGetLastError();
}
