// The KV cache as one operand of the cached-decoding entry points (decode.hip: ljs_kv_append,
// ljs_attn_decode; prefill.hip: ljs_attn_chunk), and the checks those launchers share.  Host side only.
//
// A cache is k / v buffers (B, cap, Hkv, dim) with the head dim (64 or 128) contiguous and their own (batch,
// position, head) strides, of one of two kinds:
//   bf16    k / v hold bf16; strides count ELEMENTS; no scale buffers (both scale bases null)
//   MX-fp8  k / v hold OCP e4m3 bytes and ks / vs one e8m0 byte per 32 elements, (B, cap, Hkv, dim / 32); the
//           strides of all four count BYTES
// The kind is stated, never inferred: a kind that does not match the scale bases is refused, so a null
// scale of an MX-fp8 cache cannot turn the call into a bf16 one.  ops/hip.py mirrors the struct with ctypes
// and checks its size against ljs_cache_desc_size() when the library loads.
#pragma once
#include <stdint.h>

enum { kCacheBf16 = 0, kCacheMx8 = 1 };

struct LjsCache {
  int kind, cap, Hkv;
  int dim;                  // the head dim, 64 or 128 (where the ABI pads the three ints up to the first pointer)
  void *k, *v;
  long sk[3], sv[3];
  void *ks, *vs;            // MX-fp8 only
  long sks[3], svs[3];
};

// ---- the alignment rules, each once: a non-null base on a `base`-byte boundary and the three outer strides
// multiples of `unit` (in the buffer's own stride unit)
inline bool strides_aligned(const void* p, const long* st, uintptr_t base, long unit) {
  return p && st && ((uintptr_t)p) % base == 0 && st[0] % unit == 0 && st[1] % unit == 0 && st[2] % unit == 0;
}
// bf16 rows (q, o, new k / v, a bf16 cache): everything 16-byte aligned, strides in elements
inline bool bf16_aligned(const void* p, const long* st) { return strides_aligned(p, st, 16, 8); }
// e4m3 rows of an MX-fp8 cache: everything 16-byte aligned, strides in bytes
inline bool q8_aligned(const void* p, const long* st) { return strides_aligned(p, st, 16, 16); }
// their e8m0 scales, dim / 32 bytes a row (2 at 64, 4 at 128): the base and the byte strides are multiples of
// that, so one lane stores or loads a row's scales with one access of that size
inline bool scale_aligned(const void* p, const long* st, int dim) { return strides_aligned(p, st, dim / 32, dim / 32); }

inline bool cache_dim_ok(const LjsCache& c) { return c.dim == 64 || c.dim == 128; }

// a head dim of 64 or 128, a kind in {bf16, MX-fp8}, scale bases that match it, and every buffer aligned by its rule
inline bool cache_aligned(const LjsCache& c) {
  if (!cache_dim_ok(c)) return false;
  if (c.kind == kCacheBf16) return !c.ks && !c.vs && bf16_aligned(c.k, c.sk) && bf16_aligned(c.v, c.sv);
  if (c.kind == kCacheMx8)
    return q8_aligned(c.k, c.sk) && q8_aligned(c.v, c.sv) && scale_aligned(c.ks, c.sks, c.dim) &&
           scale_aligned(c.vs, c.svs, c.dim);
  return false;
}

// rows do not overlap (a row stride of at least dim elements, dim / 32 scale bytes), and a load's byte offset
// `reach` rows into the cache (its capacity plus what the kernel reads ahead) stays a positive int
inline bool cache_reach_ok(const LjsCache& c, long reach) {
  const bool mx8 = c.kind == kCacheMx8;
  const long es = mx8 ? 1 : 2;           // bytes per cache element
  const long nsc = c.dim / 32;           // scale bytes per row
  if (c.sk[1] < c.dim || c.sv[1] < c.dim || reach * c.sk[1] * es >= 0x7fffffffL || reach * c.sv[1] * es >= 0x7fffffffL)
    return false;
  return !mx8 || !(c.sks[1] < nsc || c.svs[1] < nsc || reach * c.sks[1] >= 0x7fffffffL || reach * c.svs[1] >= 0x7fffffffL);
}
