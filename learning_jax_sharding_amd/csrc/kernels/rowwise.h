// Shared pieces of the streaming (memory-bound) kernels: 16-byte chunk I/O with the bf16
// unpack / pack, the rows-to-threads mapping of the row-wise kernels, and the in-launch
// last-arriver hand-off (norm.hip, xent.hip, loss.hip, elementwise.hip).
#pragma once
#include "common.h"

// ---- bf16 pairs <-> f32 in registers: the low half of a 32-bit word is the even element
__device__ __forceinline__ float bf16_lo(unsigned w) { return __uint_as_float(w << 16); }
__device__ __forceinline__ float bf16_hi(unsigned w) { return __uint_as_float(w & 0xffff0000u); }
__device__ __forceinline__ f32x4 unpack_bf16x4(const u32x2& a) {
  return f32x4{bf16_lo(a[0]), bf16_hi(a[0]), bf16_lo(a[1]), bf16_hi(a[1])};
}
__device__ __forceinline__ void unpack_bf16x8(const u32x4& a, float (&v)[8]) {
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    v[2 * k] = bf16_lo(a[k]);
    v[2 * k + 1] = bf16_hi(a[k]);
  }
}
__device__ __forceinline__ u32x4 pack_bf16x8(const float (&v)[8]) {
  u32x4 a;
#pragma unroll
  for (int k = 0; k < 4; ++k) a[k] = pack_bf16x2(v[2 * k], v[2 * k + 1]);
  return a;
}

// ---- one 16-byte chunk <-> E = 16 / sizeof(T) floats: 4 f32 or 8 bf16.  kAligned16 promises a
// 16-byte aligned address; kElemAligned promises only element alignment (an under-aligned
// global_load_dwordx4, which gfx9 global memory takes)
constexpr bool kAligned16 = true, kElemAligned = false;
template <typename V, bool ALIGNED>
__device__ __forceinline__ V load16(const void* p) {
  if constexpr (ALIGNED) return *reinterpret_cast<const V*>(p);
  V a;
  __builtin_memcpy(&a, p, 16);
  return a;
}
template <bool ALIGNED, typename V>
__device__ __forceinline__ void store16(void* p, const V& a) {
  if constexpr (ALIGNED) *reinterpret_cast<V*>(p) = a;
  else __builtin_memcpy(p, &a, 16);
}
template <bool ALIGNED = kAligned16>
__device__ __forceinline__ void load_chunk(const float* p, float* v) {
  const f32x4 a = load16<f32x4, ALIGNED>(p);
#pragma unroll
  for (int k = 0; k < 4; ++k) v[k] = a[k];
}
template <bool ALIGNED = kAligned16>
__device__ __forceinline__ void load_chunk(const bf16_t* p, float* v) {
  const u32x4 a = load16<u32x4, ALIGNED>(p);
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    v[2 * k] = bf16_lo(a[k]);
    v[2 * k + 1] = bf16_hi(a[k]);
  }
}
template <bool ALIGNED = kAligned16>
__device__ __forceinline__ void store_chunk(float* p, const float* v) {
  f32x4 a;
#pragma unroll
  for (int k = 0; k < 4; ++k) a[k] = v[k];
  store16<ALIGNED>(p, a);
}
template <bool ALIGNED = kAligned16>
__device__ __forceinline__ void store_chunk(bf16_t* p, const float* v) {
  u32x4 a;
#pragma unroll
  for (int k = 0; k < 4; ++k) a[k] = pack_bf16x2(v[2 * k], v[2 * k + 1]);
  store16<ALIGNED>(p, a);
}
// 8 elements: two f32 chunks (both loads issued before either is used) or one bf16 chunk
template <typename T>
__device__ __forceinline__ void load_chunk8(const T* p, float (&v)[8]) {
#pragma unroll
  for (int e = 0; e < 8; e += 16 / (int)sizeof(T)) load_chunk(p + e, v + e);
}
template <typename T>
__device__ __forceinline__ void store_chunk8(T* p, const float (&v)[8]) {
#pragma unroll
  for (int e = 0; e < 8; e += 16 / (int)sizeof(T)) store_chunk(p + e, v + e);
}

__device__ __forceinline__ float load1(const float* p) { return *p; }
__device__ __forceinline__ float load1(const bf16_t* p) { return bf2f(*p); }
__device__ __forceinline__ void store1(float* p, float v) { *p = v; }
__device__ __forceinline__ void store1(bf16_t* p, float v) { *p = f2bf(v); }

// ---- rows to threads: one wave per row with WAVES rows per block, or (BLOCK) one block of
// kRowBlockThreads per row.  A thread takes the chunks slot(), slot() + W, .. of its row and the
// rows first(), first() + step(), ..
constexpr int kRowBlockThreads = 256;
template <bool BLOCK, int WAVES>
struct RowMap {
  static constexpr int W = BLOCK ? kRowBlockThreads : 64;  // chunk stride between a thread's chunks
  __device__ static int slot() { return BLOCK ? threadIdx.x : threadIdx.x & 63; }
  __device__ static long first() { return BLOCK ? blockIdx.x : (long)blockIdx.x * WAVES + (threadIdx.x >> 6); }
  __device__ static long step() { return BLOCK ? gridDim.x : (long)gridDim.x * WAVES; }
};

// ---- in-launch "last arriver" hand-off (cdna_hip_programming.md §6 Guideline 16, the valid form
// with write-through payloads and no fences).  The contract, for n arriving blocks and one ticket:
//   before:  each block writes its payload with sc1_store only, from ONE wave (wave forms) or from
//            any of its waves (block form), and then calls lane0_last* / wave_last* from that one
//            wave, or block_last from every thread.  The form drains the stores (s_waitcnt vmcnt(0) in every storing
//            wave, a barrier where more than one wave stored) before one lane's agent-scope ticket
//            add, so a payload is in memory before its arrival can be counted.
//   after:   exactly one block, the one whose add returned n - 1, gets true (in lane 0, or
//            uniform over the wave / block).  It may read every payload of the n arrivals, with sc1_load for EVERY such
//            load (a plain load may hit a stale line in this CU's L1); the others get false and
//            must not touch the payloads.
//   tickets: live in a persistent workspace zeroed once at allocation; the last arriver re-arms the
//            word before it returns, so it is zero again when the launch ends (the next launch, or
//            a replayed graph, finds it armed).
__device__ __forceinline__ void sc1_store(float* p, float v) {
  __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ float sc1_load(const float* p) {
  return __hip_atomic_load(const_cast<float*>(p), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
// the draw itself: ONE lane, after the drain
__device__ __forceinline__ bool ticket_last(unsigned* ticket, unsigned n) {
  unsigned t = __hip_atomic_fetch_add(ticket, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  if (t == n - 1) {
    __hip_atomic_store(ticket, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    return true;
  }
  return false;
}

// Two-level arrival over n blocks: one ticket word per group of kTicketGroup blocks (t[1 + grp])
// and one top word (t[0]) drawn by each group's last arriver.  One word retires only ~88
// arrivals/us, so a few hundred blocks on a single word serialise for microseconds.  t needs
// 1 + ceil(n / kTicketGroup) words.
constexpr unsigned kTicketGroup = 32;
struct TicketGroup {
  unsigned grp, in_grp, ngrp;  // block bid's group, the blocks in that group, the groups
};
__device__ __forceinline__ TicketGroup ticket_group(unsigned bid, unsigned n) {
  const unsigned grp = bid / kTicketGroup, left = n - grp * kTicketGroup;
  return {grp, left < kTicketGroup ? left : kTicketGroup, (n + kTicketGroup - 1) / kTicketGroup};
}
__device__ __forceinline__ bool ticket_last_2lvl(unsigned* t, unsigned bid, unsigned n) {
  const TicketGroup g = ticket_group(bid, n);
  return ticket_last(t + 1 + g.grp, g.in_grp) && ticket_last(t, g.ngrp);
}

// wave forms: called by the ONE wave that stored.  lane0_last*: the drain and lane 0's draw; the
// answer is lane 0's alone, for a caller that hands it on itself (a __shared__ flag the whole block
// reads after its next barrier: a broadcast over the wave first would only add to every block's
// tail).  wave_last*: the same, broadcast to the wave.
__device__ __forceinline__ bool lane0_last(unsigned* ticket, unsigned n) {
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  return (threadIdx.x & 63) == 0 && ticket_last(ticket, n);
}
__device__ __forceinline__ bool lane0_last_2lvl(unsigned* t, unsigned bid, unsigned n) {
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  return (threadIdx.x & 63) == 0 && ticket_last_2lvl(t, bid, n);
}
__device__ __forceinline__ bool wave_last(unsigned* ticket, unsigned n) {
  return __shfl((int)lane0_last(ticket, n), 0, 64);
}
__device__ __forceinline__ bool wave_last_2lvl(unsigned* t, unsigned bid, unsigned n) {
  return __shfl((int)lane0_last_2lvl(t, bid, n), 0, 64);
}
// block form: every wave may have stored; called by every thread, thread 0 draws, the block gets
// the answer through *flag (__shared__; the first barrier also covers its reuse from call to call)
__device__ __forceinline__ bool block_last(unsigned* ticket, unsigned n, int* flag) {
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();
  if (threadIdx.x == 0) *flag = ticket_last(ticket, n);
  __syncthreads();
  return *flag;
}
