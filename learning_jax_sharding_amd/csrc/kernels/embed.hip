// Fused embedding lookup over T token rows of D features: a gather forward and a deterministic,
// atomics-free scatter-sum backward.  The table is [Vloc, D] (row stride ldt elements): the whole
// vocabulary or this device's shard of its rows; vocab_offset is the global id of the shard's row 0.
//
//   forward, per token t:   out[t] = table[ids[t] - vocab_offset], rounded once (RNE) when an f32
//                           table gives a bf16 output, a row of +0 when ids[t] - vocab_offset lies
//                           outside [0, Vloc): a negative id, an id past the vocabulary, an id that
//                           another vocabulary shard owns.  Such a token reads nothing.
//   backward:               dTable[v] = sum over the tokens t with ids[t] - vocab_offset == v of
//                           f32(dY[t]), in ascending t; rows no token chose are written as +0.
//
// Table and output are f32 or bf16 independently, ids int32 or int64, dY f32 or bf16, dTable f32.
// D is a multiple of 8 in 8..8192 (the norm kernels' rule), every base and row 16-byte aligned.
// One wave per row in both directions, 16-byte chunks, 64-bit row offsets.  With equal dtypes the
// forward moves each 16-byte chunk as bits; otherwise every value is converted once.
//
// The backward is the store pass + per-destination sum pass of a scatter-add without float atomics
// (cdna_hip_programming.md Appendix B): dY already is the stored contribution rows, so only the
// inverted index (per table row the ascending list of its tokens) and the sum pass are new.
//
//   embed_rank   rank[t] = #{t' < t : ids[t'] == ids[t]} by an all-pairs sweep: a block takes 64
//                tokens, stages the earlier ids in LDS tiles of 2048 (as local rows, int32), its four
//                waves each compare a quarter of a tile; the four counts meet in LDS.  The same
//                kernel bumps hist[row] with integer atomics, whose result no arrival order changes.
//   embed_scan   one block: start[Vloc + 1] = exclusive scan of hist, hist re-zeroed (it is a
//                persistent workspace, zero between launches), and the work list of the long lists:
//                a row with more than kEmbedChunk tokens gets one (row, chunk) item per chunk of
//                kEmbedChunk tokens, at the position a second scan gives it.
//   embed_fill   list[start[row] + rank[t]] = t.
//   embed_bwd    one wave per table row adds its list's dY rows in f32 in list order and writes the
//                row; a long row is left to the chunk items, which the first waves of the same grid
//                take: each sums one chunk, in order, into a partial row.
//   embed_combine  per long row: the partial rows added in chunk order, the row written.
//
// So dTable[v] is the f32 sequence acc = 0; acc += dY[t] over a chunk's tokens in ascending order,
// then acc = 0; acc += partial over the chunks in order (one chunk: the partial itself).  Which wave
// or block runs when changes nothing: no float atomics, no memset of the output, every row written
// exactly once, nothing to zero per call.  A long list is cut because token frequencies are
// Zipfian and a sum pass runs as long as its most loaded wave.
#include "rowwise.h"
#include <type_traits>

namespace {

#ifndef LJS_EMBED_CHUNK
#define LJS_EMBED_CHUNK 64             // (a variant build, csrc/build.py --variant, may try another)
#endif
constexpr int kEmbedChunk = LJS_EMBED_CHUNK;  // tokens of one list summed by one wave
constexpr int kAllPairsMaxT = 32768;   // most tokens the all-pairs rank is meant for (the caller sorts above)
constexpr int kWaves = 4;              // rows in flight per block (forward, sum pass)
constexpr int kBlockThreads = kRowBlockThreads;
constexpr int kFwdMaxBlocks = 8192;    // rows beyond the grid are taken by a grid-stride loop
constexpr int kMinD = 8, kMaxD = 8192;

constexpr int kRankTok = 64;           // tokens per block of the rank kernel (one per lane)
constexpr int kRankTile = 2048;        // earlier ids staged per step, a quarter per wave
constexpr int kScanThreads = 512;     // (1024 would cap a thread at 128 VGPRs: the unrolled groups spill)
constexpr int kScanTile = kScanThreads * 4;
constexpr int kScanPer = 4;            // tiles whose counts a thread loads before it scans the first

constexpr int kSumU = 2;               // sum pass: 16-byte chunks per lane per column pass
constexpr int kSumTok = 4;             // and list entries in flight

// ------------------------------------------------------------------------------------ forward
template <typename Ttab, typename Tout, typename Tid>
__global__ __launch_bounds__(kBlockThreads)
void embed_fwd_kernel(const Ttab* __restrict__ table, long ldt, const Tid* __restrict__ ids, long vocab_offset,
                      Tout* __restrict__ out, long T, int Vloc, int D) {
  using M = RowMap<false, kWaves>;
  const int slot = M::slot(), n8 = D / 8;  // groups of 8 elements
  const long step = M::step();
  for (long row = M::first(); row < T; row += step) {
    const long c = (long)ids[row] - vocab_offset;
    const bool own = c >= 0 && c < (long)Vloc;  // wave-uniform
    const Ttab* src = table + (own ? c : 0) * ldt;
    Tout* dst = out + row * (long)D;
    for (int i = slot; i < n8; i += 64) {
      if constexpr (std::is_same<Ttab, Tout>::value) {
        constexpr int N16 = 8 * (int)sizeof(Ttab) / 16;  // the bits, 16 bytes at a time
        u32x4 a[N16];
#pragma unroll
        for (int k = 0; k < N16; ++k) a[k] = u32x4{0u, 0u, 0u, 0u};
        if (own) {
#pragma unroll
          for (int k = 0; k < N16; ++k) a[k] = load16<u32x4, kAligned16>((const char*)(src + i * 8) + 16 * k);
        }
#pragma unroll
        for (int k = 0; k < N16; ++k) store16<kAligned16>((char*)(dst + i * 8) + 16 * k, a[k]);
      } else {
        float v[8];
#pragma unroll
        for (int k = 0; k < 8; ++k) v[k] = 0.f;
        if (own) load_chunk8(src + i * 8, v);
        store_chunk8(dst + i * 8, v);
      }
    }
  }
}

// ------------------------------------------------------------------------------------ index
// the table row of this shard a token chose, or none (< 0) for a token the shard does not own
template <typename Tid>
__device__ __forceinline__ int local_row(const Tid* ids, int t, long vocab_offset, int Vloc, int none) {
  const long c = (long)ids[t] - vocab_offset;
  return c >= 0 && c < (long)Vloc ? (int)c : none;
}

template <typename Tid>
__global__ __launch_bounds__(kBlockThreads)
void embed_rank_kernel(const Tid* __restrict__ ids, long vocab_offset, int T, int Vloc, int* __restrict__ rank,
                       int* __restrict__ hist) {
  __shared__ __attribute__((aligned(16))) int tile[kRankTile];
  __shared__ int part[kWaves][kRankTok];
  const int b = gridDim.x - 1 - blockIdx.x;  // the blocks with the most earlier tokens start first
  const int t0 = b * kRankTok, lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int t = t0 + lane;
  // an unowned token is -1 here and -2 in a tile: it matches nothing
  const int my = t < T ? local_row(ids, t, vocab_offset, Vloc, -1) : -1;
  int cnt = 0;
  // the tokens before the block's own, a tile at a time; the next tile's ids are loaded into
  // registers while this one is compared, so only the first load's latency is exposed
  constexpr int kPer = kRankTile / kBlockThreads;
  int nxt[kPer];
  auto fetch = [&](int base) {
#pragma unroll
    for (int k = 0; k < kPer; ++k) {
      const int tp = base + k * kBlockThreads + (int)threadIdx.x;
      nxt[k] = tp < t0 ? local_row(ids, tp, vocab_offset, Vloc, -2) : -2;
    }
  };
  if (t0 > 0) fetch(0);
  for (int base = 0; base < t0; base += kRankTile) {
    __syncthreads();
#pragma unroll
    for (int k = 0; k < kPer; ++k) tile[k * kBlockThreads + threadIdx.x] = nxt[k];
    __syncthreads();
    if (base + kRankTile < t0) fetch(base + kRankTile);
    if (base + w * (kRankTile / kWaves) < t0) {
      const int4* q = reinterpret_cast<const int4*>(tile + w * (kRankTile / kWaves));
#pragma unroll 8
      for (int j = 0; j < kRankTile / kWaves / 4; ++j) {
        const int4 v = q[j];
        cnt += (int)(v.x == my) + (int)(v.y == my) + (int)(v.z == my) + (int)(v.w == my);
      }
    }
  }
  __syncthreads();
  if (w == 0) tile[lane] = my < 0 ? -2 : my;  // the block's own tokens: those before this lane's
  __syncthreads();
  if (w == 0) {
    for (int j = 0; j < kRankTok; ++j) cnt += (int)(tile[j] == my && j < lane);
  }
  part[w][lane] = cnt;
  __syncthreads();
  if (w == 0 && t < T) {
    int r = 0;
#pragma unroll
    for (int k = 0; k < kWaves; ++k) r += part[k][lane];
    rank[t] = r;
    if (my >= 0) atomicAdd(hist + my, 1);
  }
}

__device__ __forceinline__ int chunks_of(int n) { return n > kEmbedChunk ? (n + kEmbedChunk - 1) / kEmbedChunk : 0; }

// work: [0] the number of items, [1] unused, then (row, chunk) pairs; cap: the pairs there is room for
__global__ __launch_bounds__(kScanThreads)
void embed_scan_kernel(int* __restrict__ hist, int Vloc, int* __restrict__ start, int* __restrict__ work, int cap) {
  __shared__ int wsum[2][kScanThreads / 64];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int Vpad = (Vloc + 3) & ~3;  // hist has Vpad words; the padding stays zero
  int carry = 0, wcarry = 0;
  for (int base0 = 0; base0 < Vpad; base0 += kScanTile * kScanPer) {
   int4 cs[kScanPer];
#pragma unroll
   for (int u = 0; u < kScanPer; ++u) {  // every load of the group in flight at once
     const int i = base0 + u * kScanTile + (int)threadIdx.x * 4;
     cs[u] = int4{0, 0, 0, 0};
     if (i < Vpad) {
       cs[u] = *reinterpret_cast<const int4*>(hist + i);
       *reinterpret_cast<int4*>(hist + i) = int4{0, 0, 0, 0};
     }
   }
#pragma unroll
   for (int u = 0; u < kScanPer; ++u) {
    const int i = base0 + u * kScanTile + (int)threadIdx.x * 4;
    int n[4] = {cs[u].x, cs[u].y, cs[u].z, cs[u].w}, k[4];
    int x = 0, y = 0;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      k[e] = chunks_of(n[e]);
      x += n[e];
      y += k[e];
    }
    int xs = x, ys = y;  // inclusive over the wave
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
      const int a = __shfl_up(xs, o, 64), c = __shfl_up(ys, o, 64);
      if (lane >= o) { xs += a; ys += c; }
    }
    if (lane == 63) { wsum[0][w] = xs; wsum[1][w] = ys; }
    __syncthreads();
    int px = carry + xs - x, py = wcarry + ys - y, tx = 0, ty = 0;
#pragma unroll
    for (int j = 0; j < kScanThreads / 64; ++j) {
      const int a = wsum[0][j], c = wsum[1][j];
      if (j < w) { px += a; py += c; }
      tx += a;
      ty += c;
    }
    __syncthreads();
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const int v = i + e;
      if (v < Vloc) {
        start[v] = px;
        for (int kk = 0; kk < k[e]; ++kk) {
          const int s = py + kk;
          if (s >= 0 && s < cap) { work[2 + 2 * s] = v; work[3 + 2 * s] = kk; }
        }
        px += n[e];
        py += k[e];
      }
    }
    carry += tx;
    wcarry += ty;
   }
  }
  if (threadIdx.x == 0) {
    start[Vloc] = carry;
    work[0] = wcarry < 0 ? 0 : (wcarry < cap ? wcarry : cap);
  }
}

template <typename Tid>
__global__ __launch_bounds__(kBlockThreads)
void embed_fill_kernel(const Tid* __restrict__ ids, long vocab_offset, int T, int Vloc, const int* __restrict__ rank,
                       const int* __restrict__ start, int* __restrict__ list) {
  for (int t = blockIdx.x * kBlockThreads + threadIdx.x; t < T; t += gridDim.x * kBlockThreads) {
    const int c = local_row(ids, t, vocab_offset, Vloc, -1);
    if (c >= 0) {
      const int p = start[c] + rank[t];
      if ((unsigned)p < (unsigned)T) list[p] = t;
    }
  }
}

// ------------------------------------------------------------------------------------ sum pass
__device__ __forceinline__ int clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

// dst[D] (f32) = the dY rows list[j0 .. j1) added in that order from 0, by one wave.  A lane keeps
// kSumU chunks of the row in registers, so a row wider than 64 kSumU chunks takes several passes
// over the list.
template <typename Tdy>
__device__ __forceinline__ void sum_list(const Tdy* __restrict__ dy, int D, int T, const int* __restrict__ list,
                                         int j0, int j1, float* __restrict__ dst) {
  constexpr int E = 16 / (int)sizeof(Tdy);
  const int lane = threadIdx.x & 63, nvec = D / E;
  for (int c0 = 0; c0 < nvec; c0 += 64 * kSumU) {
    float acc[kSumU][E];
#pragma unroll
    for (int u = 0; u < kSumU; ++u)
#pragma unroll
      for (int e = 0; e < E; ++e) acc[u][e] = 0.f;
    for (int jb = j0; jb < j1; jb += 64) {
      const int nb = j1 - jb < 64 ? j1 - jb : 64;
      int tl = lane < nb ? list[jb + lane] : 0;
      tl = (unsigned)tl < (unsigned)T ? tl : 0;  // never an address outside dY
      int k = 0;
      for (; k + kSumTok <= nb; k += kSumTok) {
        float v[kSumTok][kSumU][E];
#pragma unroll
        for (int q = 0; q < kSumTok; ++q) {
          const Tdy* p = dy + (long)__shfl(tl, k + q, 64) * D;
#pragma unroll
          for (int u = 0; u < kSumU; ++u) {
            const int i = c0 + lane + u * 64;
            if (i < nvec) load_chunk(p + (long)i * E, v[q][u]);
          }
        }
#pragma unroll
        for (int q = 0; q < kSumTok; ++q)
#pragma unroll
          for (int u = 0; u < kSumU; ++u) {
            if (c0 + lane + u * 64 < nvec) {
#pragma unroll
              for (int e = 0; e < E; ++e) acc[u][e] += v[q][u][e];
            }
          }
      }
      for (; k < nb; ++k) {
        const Tdy* p = dy + (long)__shfl(tl, k, 64) * D;
        float v[kSumU][E];
#pragma unroll
        for (int u = 0; u < kSumU; ++u) {
          const int i = c0 + lane + u * 64;
          if (i < nvec) load_chunk(p + (long)i * E, v[u]);
        }
#pragma unroll
        for (int u = 0; u < kSumU; ++u) {
          if (c0 + lane + u * 64 < nvec) {
#pragma unroll
            for (int e = 0; e < E; ++e) acc[u][e] += v[u][e];
          }
        }
      }
    }
#pragma unroll
    for (int u = 0; u < kSumU; ++u) {
      const int i = c0 + lane + u * 64;
      if (i < nvec) {
#pragma unroll
        for (int e = 0; e < E; e += 4) store_chunk(dst + (long)i * E + e, acc[u] + e);
      }
    }
  }
}

// waves [0, cap): the chunk items of the long lists (the heaviest work, started first); waves
// cap + v: table row v
template <typename Tdy>
__global__ __launch_bounds__(kBlockThreads)
void embed_bwd_kernel(const Tdy* __restrict__ dy, int D, int T, int Vloc, const int* __restrict__ start,
                      const int* __restrict__ list, const int* __restrict__ work, int cap,
                      float* __restrict__ partial, float* __restrict__ dtable) {
  const long gw = (long)blockIdx.x * kWaves + (threadIdx.x >> 6);
  if (gw < cap) {
    const int s = (int)gw;
    if (s >= work[0]) return;
    const int v = work[2 + 2 * s], k = work[3 + 2 * s];
    if ((unsigned)v >= (unsigned)Vloc || k < 0) return;
    const int end = clampi(start[v + 1], 0, T);
    const int a = clampi(start[v] + k * kEmbedChunk, 0, end);
    const int b = a + kEmbedChunk < end ? a + kEmbedChunk : end;
    sum_list(dy, D, T, list, a, b, partial + (long)s * D);
    return;
  }
  const long v = gw - cap;
  if (v >= Vloc) return;
  const int b = clampi(start[v + 1], 0, T), a = clampi(start[v], 0, b);
  if (b - a > kEmbedChunk && cap > 0) return;  // a long list: its chunk items and embed_combine
  sum_list(dy, D, T, list, a, b, dtable + v * D);
}

// one wave per work item; the item of a row's chunk 0 adds the row's partials in chunk order
__global__ __launch_bounds__(kBlockThreads)
void embed_combine_kernel(int D, int Vloc, const int* __restrict__ start, const int* __restrict__ work, int cap,
                          const float* __restrict__ partial, float* __restrict__ dtable) {
  const int s = blockIdx.x * kWaves + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (s >= cap || s >= work[0] || work[3 + 2 * s] != 0) return;
  const int v = work[2 + 2 * s];
  if ((unsigned)v >= (unsigned)Vloc) return;
  int nch = chunks_of(start[v + 1] - start[v]);
  if (s + nch > cap) nch = cap - s;
  for (int i = lane; i < D / 4; i += 64) {
    float acc[4] = {0.f, 0.f, 0.f, 0.f};
    for (int c = 0; c < nch; ++c) {
      float p[4];
      load_chunk(partial + (long)(s + c) * D + i * 4, p);
#pragma unroll
      for (int e = 0; e < 4; ++e) acc[e] += p[e];
    }
    store_chunk(dtable + (long)v * D + i * 4, acc);
  }
}

inline bool aligned16(const void* p) { return (((uintptr_t)p) & 15u) == 0; }
inline bool dim_ok(int D) { return D % 8 == 0 && D >= kMinD && D <= kMaxD; }
inline unsigned waves_grid(long waves) { return (unsigned)((waves + kWaves - 1) / kWaves); }

template <typename Ttab, typename Tout, typename Tid>
int launch_fwd(const char* name, const void* table, long ldt, const void* ids, long vocab_offset, void* out, long T,
               int Vloc, int D, hipStream_t st) {
  const long g = (T + kWaves - 1) / kWaves;
  const dim3 grid((unsigned)(g < kFwdMaxBlocks ? g : kFwdMaxBlocks));
  hipLaunchKernelGGL((embed_fwd_kernel<Ttab, Tout, Tid>), grid, dim3(kBlockThreads), 0, st, (const Ttab*)table, ldt,
                     (const Tid*)ids, vocab_offset, (Tout*)out, T, Vloc, D);
  ljs_launch_rec(name, grid, kBlockThreads);
  return (int)hipGetLastError();
}

template <typename Tid>
int launch_index(const void* ids, long vocab_offset, int T, int Vloc, int* hist, int* rank, int* start, int* list,
                 int* work, int cap, hipStream_t st) {
  const dim3 gr((unsigned)((T + kRankTok - 1) / kRankTok));
  hipLaunchKernelGGL((embed_rank_kernel<Tid>), gr, dim3(kBlockThreads), 0, st, (const Tid*)ids, vocab_offset, T, Vloc,
                     rank, hist);
  ljs_launch_rec("embed_rank", gr, kBlockThreads);
  hipLaunchKernelGGL(embed_scan_kernel, dim3(1), dim3(kScanThreads), 0, st, hist, Vloc, start, work, cap);
  ljs_launch_rec("embed_scan", dim3(1), kScanThreads);
  const int fb = (T + kBlockThreads - 1) / kBlockThreads;
  const dim3 gf((unsigned)(fb < 1024 ? fb : 1024));
  hipLaunchKernelGGL((embed_fill_kernel<Tid>), gf, dim3(kBlockThreads), 0, st, (const Tid*)ids, vocab_offset, T, Vloc,
                     rank, start, list);
  ljs_launch_rec("embed_fill", gf, kBlockThreads);
  return (int)hipGetLastError();
}

template <typename Tdy>
int launch_bwd(const char* name, const void* dy, int D, int T, int Vloc, const int* start, const int* list,
               const int* work, int cap, float* partial, float* dtable, hipStream_t st) {
  const dim3 grid(waves_grid((long)cap + Vloc));
  hipLaunchKernelGGL((embed_bwd_kernel<Tdy>), grid, dim3(kBlockThreads), 0, st, (const Tdy*)dy, D, T, Vloc, start, list,
                     work, cap, partial, dtable);
  ljs_launch_rec(name, grid, kBlockThreads);
  if (cap > 0) {
    const dim3 gc(waves_grid(cap));
    hipLaunchKernelGGL(embed_combine_kernel, gc, dim3(kBlockThreads), 0, st, D, Vloc, start, work, cap,
                       (const float*)partial, dtable);
    ljs_launch_rec("embed_combine", gc, kBlockThreads);
  }
  return (int)hipGetLastError();
}

}  // namespace

// tokens of one list summed by one wave: a longer list is cut into chunks of this many, in order
LJS_API int ljs_embed_chunk() { return kEmbedChunk; }
// most tokens ljs_embed_index is meant for; above, the caller builds the index from a stable sort
LJS_API int ljs_embed_allpairs_max_tokens() { return kAllPairsMaxT; }
// (row, chunk) items that T tokens can give: a long row has more than kEmbedChunk tokens, so
// sum ceil(n / chunk) over the long rows < 2 T / chunk.  0: no list can be long.
LJS_API int ljs_embed_work_cap(long T) { return T > kEmbedChunk ? (int)(2 * (T / kEmbedChunk) + 2) : 0; }

// table: [Vloc] rows of D f32 or bf16, row stride ldt elements; ids: [T] int32 or int64 global ids;
// out: [T, D] contiguous f32 or bf16.
LJS_API int ljs_embed_fwd(const void* table, int table_bf16, long ldt, const void* ids, int ids_i64,
                          long vocab_offset, void* out, int out_bf16, long T, int Vloc, int D, hipStream_t st) {
  const int ts = table_bf16 ? 2 : 4;
  if (!table || !ids || !out || T < 1 || Vloc < 1 || !dim_ok(D) || ldt < D || (ldt * ts) % 16 != 0 ||
      !aligned16(table) || !aligned16(out))
    return (int)hipErrorInvalidValue;
#define LJS_EMBED_CASE(TT, TS, TO, OS, TI)                                                                     \
  if ((table_bf16 != 0) == std::is_same<TT, bf16_t>::value && (out_bf16 != 0) == std::is_same<TO, bf16_t>::value && \
      (ids_i64 != 0) == std::is_same<TI, long>::value)                                                         \
    return launch_fwd<TT, TO, TI>("embed_fwd<" TS "," OS ">", table, ldt, ids, vocab_offset, out, T, Vloc, D, st);
#define LJS_EMBED_IDS(TT, TS, TO, OS) LJS_EMBED_CASE(TT, TS, TO, OS, int) LJS_EMBED_CASE(TT, TS, TO, OS, long)
  LJS_EMBED_IDS(float, "f32", float, "f32")
  LJS_EMBED_IDS(float, "f32", bf16_t, "bf16")
  LJS_EMBED_IDS(bf16_t, "bf16", float, "f32")
  LJS_EMBED_IDS(bf16_t, "bf16", bf16_t, "bf16")
#undef LJS_EMBED_IDS
#undef LJS_EMBED_CASE
  return (int)hipErrorInvalidValue;
}

// The inverted index of ids[T] over this shard's rows: start[Vloc + 1], list[T] (its first
// start[Vloc] entries: the owned tokens, by row, ascending inside a row) and the work list of the
// long rows (2 + 2 cap ints, cap = ljs_embed_work_cap(T)).  hist: (Vloc + 3) / 4 * 4 ints, zero on
// entry and zero again when the launches end; rank: T ints of scratch.
LJS_API int ljs_embed_index(const void* ids, int ids_i64, long vocab_offset, long T, int Vloc, void* hist, void* rank,
                            void* start, void* list, void* work, int cap, hipStream_t st) {
  if (!ids || !hist || !rank || !start || !list || !work || T < 1 || T >= (1L << 31) - kRankTile || Vloc < 1 ||
      cap < 0 || !aligned16(hist))
    return (int)hipErrorInvalidValue;
  if (ids_i64)
    return launch_index<long>(ids, vocab_offset, (int)T, Vloc, (int*)hist, (int*)rank, (int*)start, (int*)list,
                              (int*)work, cap, st);
  return launch_index<int>(ids, vocab_offset, (int)T, Vloc, (int*)hist, (int*)rank, (int*)start, (int*)list,
                           (int*)work, cap, st);
}

// The scan alone, for an index whose list comes from a stable sort: hist holds the rows' token
// counts (and is zeroed); writes start and the work list.
LJS_API int ljs_embed_scan(void* hist, int Vloc, void* start, void* work, int cap, hipStream_t st) {
  if (!hist || !start || !work || Vloc < 1 || cap < 0 || !aligned16(hist)) return (int)hipErrorInvalidValue;
  hipLaunchKernelGGL(embed_scan_kernel, dim3(1), dim3(kScanThreads), 0, st, (int*)hist, Vloc, (int*)start, (int*)work,
                     cap);
  ljs_launch_rec("embed_scan", dim3(1), kScanThreads);
  return (int)hipGetLastError();
}

// dtable: [Vloc, D] f32 contiguous, every row written; dy: [T, D] contiguous f32 or bf16;
// partial: cap * D floats of scratch (null when cap is 0).
LJS_API int ljs_embed_bwd(const void* dy, int dy_bf16, long T, int D, int Vloc, const void* start, const void* list,
                          const void* work, int cap, void* partial, void* dtable, hipStream_t st) {
  if (!dy || !start || !list || !work || !dtable || T < 1 || T >= (1L << 31) || Vloc < 1 || !dim_ok(D) || cap < 0 ||
      (cap > 0 && !partial) || !aligned16(dy) || !aligned16(dtable) || !aligned16(partial))
    return (int)hipErrorInvalidValue;
  if (dy_bf16)
    return launch_bwd<bf16_t>("embed_bwd<bf16>", dy, D, (int)T, Vloc, (const int*)start, (const int*)list,
                              (const int*)work, cap, (float*)partial, (float*)dtable, st);
  return launch_bwd<float>("embed_bwd<f32>", dy, D, (int)T, Vloc, (const int*)start, (const int*)list,
                           (const int*)work, cap, (float*)partial, (float*)dtable, st);
}
