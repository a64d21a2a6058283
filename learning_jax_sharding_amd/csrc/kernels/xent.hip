// Fused softmax cross-entropy with integer labels over R rows (tokens) of V contiguous logits
// (row stride ld >= V elements), forward and backward in one streaming pass each.  V is the whole
// vocabulary or this device's shard of it; vocab_offset is the global index of the shard's column 0.
//
//   forward, per row:   m = max x,   s = sum exp(x - m),   t = x[label] - m if this shard owns the
//                       label (vocab_offset <= label < vocab_offset + V), else 0,
//                       loss = log(s) - t  (optional; the whole-vocabulary case)
//   backward, per row:  dx[c] = a exp(x[c] - m) / s - b [c + vocab_offset == label]
//
// A label < 0 marks an ignored row: loss 0, dx row 0.  Logits (and dx) are f32 or bf16, labels
// int32 or int64, every statistic and all arithmetic f32.  The maximum and the sum stay two values
// from the per-thread online softmax to the outputs: log-sum-exp is never formed, so a loss of
// order 1 is never the difference of two numbers of the logits' magnitude.
//
// exp(x - m) is a raw exp2 of fma(x, log2e, -mh) - dl with mh = fl(m log2e) and dl = m log2e - mh
// = fma(m, log2e, -mh), exact: mh alone is off from m log2e by up to half an ulp (7.6e-6 for logits
// near 100), which would scale every term of a row by 2^dl; with dl taken off, x = m gives
// exp2(0) = 1 exactly, so a one-column row has s = 1, loss 0 and dx 0 as in exact arithmetic.
// Contraction is off in this file so that mh is the same rounded product wherever it is formed;
// the FMAs are explicit.
//
// Any V >= 1 and any element-aligned base and stride: a row is V / E whole chunks of E = 16 bytes
// / element size columns, counted from column 0, and a tail of V % E single elements taken by the
// first lanes; kU chunks are in flight per thread.  Chunk j is one 16-byte load (store) at column
// j E whatever the row's address: aligned wherever base and stride put rows on 16-byte boundaries,
// else an under-aligned global_load_dwordx4, which gfx9 global memory takes at element alignment.
// The split follows the columns, not the addresses, on purpose: which lane adds which column, and
// in what order, is then a function of V alone, so a strided view and its contiguous copy (whose
// rows sit differently on the 16-byte grid) give the same bits.  Peeling a head up to the row's
// first 16-byte boundary would make the order of the sum depend on the address.  Nothing outside
// [0, V) of a row is read or written.
//
// Two mappings of rows to threads, chosen by V alone (kWaveMaxV):
//   wave  (V <= 2048): one wave per row, four rows per block; (m, s) pairs merge by shuffles.
//   block (V  > 2048): one 256-thread block per row; the four waves' pairs meet in 8 floats of LDS.
// A row is never split over blocks.  Every output is per row: no atomics, no workspace, no memset,
// the same bits on every run, nothing to re-arm for a graph replay.  Row offsets are 64-bit.
#include "rowwise.h"
#include <type_traits>

#pragma clang fp contract(off)

namespace {

constexpr int kWaveMaxV = 2048;     // widest row of the wave mapping
constexpr int kWaves = 4;           // wave mapping: waves (= rows in flight) per block
constexpr int kBlockThreads = kRowBlockThreads;  // both mappings
constexpr int kMaxBlocks = 2048;    // rows beyond the grid are taken by a grid-stride loop
constexpr int kU = 4;               // 16-byte chunks in flight per thread
constexpr float kLog2e = 1.4426950408889634f;
constexpr float kNegInf = -__builtin_inff();

__device__ __forceinline__ float raw_exp2(float x) { return __builtin_amdgcn_exp2f(x); }

// running maximum m, nm = -fl(m log2e), dl = m log2e + nm, and s = sum exp(x - m) of the elements
// seen.  Before the first finite element m = -inf with nm = dl = 0: an element of -inf then adds
// exp2(-inf + 0) = 0, never exp2(-inf + inf).
struct MS {
  float m, nm, dl, s;
};

// exp(x - m) for the maximum m that nm and dl were made from
__device__ __forceinline__ float exp_rel(float x, float nm, float dl) {
  return raw_exp2(fmaf(x, kLog2e, nm) - dl);
}

template <int N>
__device__ __forceinline__ void ms_update(MS& st, const float* v) {
  float cm = v[0];
#pragma unroll
  for (int k = 1; k < N; ++k) cm = fmaxf(cm, v[k]);
  if (cm > st.m) {
    const float nm = -(cm * kLog2e), dl = fmaf(cm, kLog2e, nm);
    st.s *= exp_rel(st.m, nm, dl);  // the first time: 0 * exp2(-inf)
    st.m = cm;
    st.nm = nm;
    st.dl = dl;
  }
#pragma unroll
  for (int k = 0; k < N; ++k) st.s += exp_rel(v[k], st.nm, st.dl);
}

// (m, s) of the union of two element sets; symmetric in its arguments bit for bit
__device__ __forceinline__ void ms_merge(float& m, float& s, float m2, float s2) {
  const float M = fmaxf(m, m2), nm = -(M * kLog2e), dl = fmaf(M, kLog2e, nm);
  const float f1 = m == M ? 1.f : exp_rel(m, nm, dl);
  const float f2 = m2 == M ? 1.f : exp_rel(m2, nm, dl);
  s = s * f1 + s2 * f2;
  m = M;
}

template <typename T, typename L, bool BLOCK>
__global__ __launch_bounds__(kBlockThreads)
void xent_fwd_kernel(const T* __restrict__ x, long ld, const L* __restrict__ labels, long vocab_offset,
                     float* __restrict__ m_out, float* __restrict__ s_out, float* __restrict__ t_out,
                     float* __restrict__ loss, long R, int V) {
  using M = RowMap<BLOCK, kWaves>;
  constexpr int E = 16 / (int)sizeof(T), W = M::W;
  __shared__ float red[2][2][4];  // [row parity][m, s][wave]
  const int slot = M::slot();
  const long step = M::step();
  int par = 0;
  for (long row = M::first(); row < R; row += step, par ^= 1) {
    const T* p = x + row * ld;
    const long lab = (long)labels[row];
    const long c = lab - vocab_offset;
    const bool own = lab >= 0 && c >= 0 && c < (long)V;
    const float xl = own ? load1(p + c) : 0.f;
    const int nvec = V / E;
    MS st = {kNegInf, 0.f, 0.f, 0.f};
    for (int i0 = slot; i0 < nvec; i0 += W * kU) {
      float v[kU * E];
#pragma unroll
      for (int u = 0; u < kU; ++u) {
        const int i = i0 + u * W;
        if (i < nvec) {
          load_chunk<kElemAligned>(p + (long)i * E, v + u * E);
        } else {
#pragma unroll
          for (int k = 0; k < E; ++k) v[u * E + k] = kNegInf;  // adds exp2(-inf) = 0
        }
      }
      ms_update<kU * E>(st, v);
    }
    if (nvec * E + slot < V) {  // the tail: one element each for the first V % E lanes
      const float v = load1(p + nvec * E + slot);
      ms_update<1>(st, &v);
    }
    float m = st.m, s = st.s;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) ms_merge(m, s, __shfl_xor(m, o, 64), __shfl_xor(s, o, 64));
    if constexpr (BLOCK) {
      // alternating between two sets: a wave already writing the row after next cannot overtake
      // one still reading this one (the barrier of the row between lies in between)
      const int w = threadIdx.x >> 6;
      if ((threadIdx.x & 63) == 0) { red[par][0][w] = m; red[par][1][w] = s; }
      __syncthreads();
      m = red[par][0][0];
      s = red[par][1][0];
#pragma unroll
      for (int k = 1; k < 4; ++k) ms_merge(m, s, red[par][0][k], red[par][1][k]);
    }
    if (slot == 0) {
      const float t = own ? xl - m : 0.f;
      m_out[row] = m;
      s_out[row] = s;
      t_out[row] = t;
      if (loss) loss[row] = lab < 0 ? 0.f : logf(s) - t;
    }
  }
}

template <typename T, typename L, bool BLOCK>
__global__ __launch_bounds__(kBlockThreads)
void xent_bwd_kernel(const T* __restrict__ x, long ld, const L* __restrict__ labels, long vocab_offset,
                     const float* __restrict__ m_in, const float* __restrict__ s_in, const float* __restrict__ a_in,
                     const float* __restrict__ b_in, T* __restrict__ dx, long lddx, long R, int V) {
  using M = RowMap<BLOCK, kWaves>;
  constexpr int E = 16 / (int)sizeof(T), W = M::W;
  const int slot = M::slot();
  const long step = M::step();
  long row = M::first();
  for (; row < R; row += step) {
    const T* p = x + row * ld;
    T* q = dx + row * lddx;
    const long lab = (long)labels[row];
    const int nvec = V / E, te = nvec * E + slot;  // te: this lane's tail element, if < V
    if (lab < 0) {  // an ignored row: zeros, x is not read
      float z[E];
#pragma unroll
      for (int k = 0; k < E; ++k) z[k] = 0.f;
      for (int i = slot; i < nvec; i += W) store_chunk<kElemAligned>(q + (long)i * E, z);
      if (te < V) store1(q + te, 0.f);
      continue;
    }
    const long c = lab - vocab_offset;
    const int cl = c >= 0 && c < (long)V ? (int)c : -1;  // the label's column in this shard
    const float m = m_in[row], nm = -(m * kLog2e), dl = fmaf(m, kLog2e, nm);
    const float r = a_in[row] / s_in[row];
    const float b = b_in[row];
    if (te < V) store1(q + te, r * exp_rel(load1(p + te), nm, dl) - (te == cl ? b : 0.f));
    for (int i0 = slot; i0 < nvec; i0 += W * kU) {
      float v[kU * E];
#pragma unroll
      for (int u = 0; u < kU; ++u) {
        const int i = i0 + u * W;
        if (i < nvec) load_chunk<kElemAligned>(p + (long)i * E, v + u * E);
      }
#pragma unroll
      for (int u = 0; u < kU; ++u) {
        const int i = i0 + u * W;
        if (i < nvec) {
          float o[E];
#pragma unroll
          for (int k = 0; k < E; ++k) o[k] = r * exp_rel(v[u * E + k], nm, dl);
          const int c0 = i * E;
          if ((unsigned)(cl - c0) < (unsigned)E) {  // one chunk of the row
#pragma unroll
            for (int k = 0; k < E; ++k) o[k] -= c0 + k == cl ? b : 0.f;
          }
          store_chunk<kElemAligned>(q + (long)i * E, o);
        }
      }
    }
  }
}

inline bool block_mapping(int V) { return V > kWaveMaxV; }

inline unsigned xent_grid(long R, bool block) {
  const long g = block ? R : (R + kWaves - 1) / kWaves;
  return (unsigned)(g < kMaxBlocks ? g : kMaxBlocks);
}

template <typename T, typename L>
int launch_fwd(const char* wave_name, const char* block_name, const void* x, long ld, const void* labels,
               long vocab_offset, void* m, void* s, void* t, void* loss, long R, int V, hipStream_t st) {
  const bool block = block_mapping(V);
  const dim3 grid(xent_grid(R, block));
#define LJS_XENT_FWD(BLOCK)                                                                                      \
  hipLaunchKernelGGL((xent_fwd_kernel<T, L, BLOCK>), grid, dim3(kBlockThreads), 0, st, (const T*)x, ld,          \
                     (const L*)labels, vocab_offset, (float*)m, (float*)s, (float*)t, (float*)loss, R, V)
  if (block) LJS_XENT_FWD(true);
  else LJS_XENT_FWD(false);
#undef LJS_XENT_FWD
  ljs_launch_rec(block ? block_name : wave_name, grid, kBlockThreads);
  return (int)hipGetLastError();
}

template <typename T, typename L>
int launch_bwd(const char* wave_name, const char* block_name, const void* x, long ld, const void* labels,
               long vocab_offset, const void* m, const void* s, const void* a, const void* b, void* dx, long lddx,
               long R, int V, hipStream_t st) {
  const bool block = block_mapping(V);
  const dim3 grid(xent_grid(R, block));
#define LJS_XENT_BWD(BLOCK)                                                                                      \
  hipLaunchKernelGGL((xent_bwd_kernel<T, L, BLOCK>), grid, dim3(kBlockThreads), 0, st, (const T*)x, ld,          \
                     (const L*)labels, vocab_offset, (const float*)m, (const float*)s, (const float*)a,          \
                     (const float*)b, (T*)dx, lddx, R, V)
  if (block) LJS_XENT_BWD(true);
  else LJS_XENT_BWD(false);
#undef LJS_XENT_BWD
  ljs_launch_rec(block ? block_name : wave_name, grid, kBlockThreads);
  return (int)hipGetLastError();
}

inline bool elem_aligned(const void* p, int elem) { return (((uintptr_t)p) & (uintptr_t)(elem - 1)) == 0; }

}  // namespace

// widest row (elements) that takes the wave mapping
LJS_API int ljs_xent_wave_max_v() { return kWaveMaxV; }

// x: [R] rows of V logits, f32 or bf16, row stride ld elements; labels: [R] int32 or int64 global
// column indices (< 0: ignored row); m, s, t: f32 [R]; loss: f32 [R] or null.
LJS_API int ljs_xent_fwd(const void* x, int x_bf16, long ld, const void* labels, int labels_i64, long vocab_offset,
                         void* m, void* s, void* t, void* loss, long R, int V, hipStream_t st) {
  if (!x || !labels || !m || !s || !t || R < 1 || V < 1 || ld < V || !elem_aligned(x, x_bf16 ? 2 : 4))
    return (int)hipErrorInvalidValue;
#define LJS_XENT_CASE(T, TS, L)                                                                              \
  if ((x_bf16 != 0) == std::is_same<T, bf16_t>::value && (labels_i64 != 0) == std::is_same<L, long>::value) \
    return launch_fwd<T, L>("xent_fwd<" TS ",wave>", "xent_fwd<" TS ",block>", x, ld, labels, vocab_offset, m, s, \
                            t, loss, R, V, st);
  LJS_XENT_CASE(float, "f32", int)
  LJS_XENT_CASE(float, "f32", long)
  LJS_XENT_CASE(bf16_t, "bf16", int)
  LJS_XENT_CASE(bf16_t, "bf16", long)
#undef LJS_XENT_CASE
  return (int)hipErrorInvalidValue;
}

// dx (x's dtype, row stride lddx) = a exp(x - m) / s - b [column == label]; m, s, a, b: f32 [R].
LJS_API int ljs_xent_bwd(const void* x, int x_bf16, long ld, const void* labels, int labels_i64, long vocab_offset,
                         const void* m, const void* s, const void* a, const void* b, void* dx, long lddx, long R,
                         int V, hipStream_t st) {
  if (!x || !labels || !m || !s || !a || !b || !dx || R < 1 || V < 1 || ld < V || lddx < V ||
      !elem_aligned(x, x_bf16 ? 2 : 4) || !elem_aligned(dx, x_bf16 ? 2 : 4))
    return (int)hipErrorInvalidValue;
#define LJS_XENT_CASE(T, TS, L)                                                                              \
  if ((x_bf16 != 0) == std::is_same<T, bf16_t>::value && (labels_i64 != 0) == std::is_same<L, long>::value) \
    return launch_bwd<T, L>("xent_bwd<" TS ",wave>", "xent_bwd<" TS ",block>", x, ld, labels, vocab_offset, m, s, \
                            a, b, dx, lddx, R, V, st);
  LJS_XENT_CASE(float, "f32", int)
  LJS_XENT_CASE(float, "f32", long)
  LJS_XENT_CASE(bf16_t, "bf16", int)
  LJS_XENT_CASE(bf16_t, "bf16", long)
#undef LJS_XENT_CASE
  return (int)hipErrorInvalidValue;
}
