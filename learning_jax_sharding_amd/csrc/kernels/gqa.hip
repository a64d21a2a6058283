// Grouped-query attention: the fold of per-query-head dK / dV over each key/value head's group.
//
// With H query heads sharing Hkv = H / G key/value heads (query head h reads K/V head h / G,
// attention.hip), the backward kernels write the gradient of every QUERY head's view of K and V:
// dKx, dVx of (B, Sk, H, 64) bf16.  The gradient of key/value head j is the sum over its group:
//
//     dK[b][s][j][:] = bf16( sum over g = 0 .. G-1, in ascending g, of f32(dKx[b][s][j G + g][:]) )
//
// and the same for dV; both tensors are folded in one launch.  Plain f32 adds in that fixed order and
// one round-to-nearest-even, so the result is the same bits on every run and for every grid.
//
// One work item is (tensor, batch, key, kv head, chunk): one 16-byte chunk (8 bf16) of one output
// head row, read G times and written once.  The chunk index runs fastest, so a wave reads and
// writes whole 128-byte head rows.  Items are taken grid-stride over a grid sized from the CU
// count.  No LDS, no cross-lane traffic, no atomics, no memset.  Sources and destinations take their
// own (batch, seq, head) strides in elements (column blocks of a wider buffer, seq-major storage);
// every base and stride is 16-byte aligned and offsets are 64-bit.
#include "rowwise.h"

namespace {

constexpr int kGqaThreads = kRowBlockThreads;
constexpr int kGqaBlocksPerCu = 8;      // 8 blocks x 4 waves: every wave slot of a CU
constexpr int kGqaD = 64;               // head dim
constexpr int kGqaChunks = kGqaD / 8;   // 16-byte chunks per head row

int g_gqa_max_blocks = 0;               // > 0: a grid cap for tests (grid-stride on small shapes)

struct GqaTensor {
  bf16_t* p;
  long sb, ss, sh;                      // strides (elements): batch, key, head
};

struct GqaArgs {
  GqaTensor src[2], dst[2];             // [0]: dKx -> dK, [1]: dVx -> dV
  long per;                             // items per tensor: B Sk Hkv chunks
  int Sk, Hkv, G;
};

__global__ __launch_bounds__(kGqaThreads)
void gqa_reduce_kernel(const GqaArgs a) {
  const long step = (long)gridDim.x * kGqaThreads;
  for (long item = (long)blockIdx.x * kGqaThreads + threadIdx.x; item < 2 * a.per; item += step) {
    const int t = item >= a.per;
    long r = item - (t ? a.per : 0);
    const int c = (int)(r % kGqaChunks);
    r /= kGqaChunks;
    const int j = (int)(r % a.Hkv);
    r /= a.Hkv;
    const int s = (int)(r % a.Sk);
    const long b = r / a.Sk;
    const GqaTensor& x = a.src[t];
    const GqaTensor& y = a.dst[t];
    const bf16_t* sp = x.p + b * x.sb + (long)s * x.ss + (long)j * a.G * x.sh + c * 8;
    float acc[8], v[8];
    load_chunk(sp, acc);
    for (int g = 1; g < a.G; ++g) {
      load_chunk(sp + (long)g * x.sh, v);
#pragma unroll
      for (int e = 0; e < 8; ++e) acc[e] += v[e];
    }
    store_chunk(y.p + b * y.sb + (long)s * y.ss + (long)j * y.sh + c * 8, acc);
  }
}

inline bool gqa_aligned(const void* p, const long* st) {
  return p && st && (((uintptr_t)p) & 15u) == 0 && st[0] % 8 == 0 && st[1] % 8 == 0 && st[2] % 8 == 0;
}
inline GqaTensor gqa_tensor(const void* p, const long* st) {
  return GqaTensor{(bf16_t*)const_cast<void*>(p), st[0], st[1], st[2]};
}

}  // namespace

// tests: at most n blocks per launch (the grid-stride loop on small shapes); n <= 0: the default,
// kGqaBlocksPerCu blocks per compute unit
LJS_API int ljs_gqa_set_max_blocks(int n) {
  g_gqa_max_blocks = n > 0 ? n : 0;
  return 0;
}

// dkx, dvx (B, Sk, H, 64) bf16 -> dk, dv (B, Sk, Hkv, 64) bf16, summed over each group of H / Hkv
// adjacent heads (see the head of the file).  sxk / sxv / sdk / sdv: the (batch, seq, head) strides
// in elements.  Returns hipErrorInvalidValue, and launches and records nothing, for Hkv <= 0,
// H % Hkv != 0, an empty shape, or a base or stride that is not 16-byte aligned.
LJS_API int ljs_gqa_reduce(const void* dkx, const void* dvx, void* dk, void* dv, int B, int Sk, int H, int Hkv,
                           const long* sxk, const long* sxv, const long* sdk, const long* sdv, hipStream_t st) {
  if (B < 1 || Sk < 1 || H < 1 || Hkv < 1 || H % Hkv != 0) return (int)hipErrorInvalidValue;
  if (!gqa_aligned(dkx, sxk) || !gqa_aligned(dvx, sxv) || !gqa_aligned(dk, sdk) || !gqa_aligned(dv, sdv))
    return (int)hipErrorInvalidValue;
  GqaArgs a{};
  a.src[0] = gqa_tensor(dkx, sxk);
  a.src[1] = gqa_tensor(dvx, sxv);
  a.dst[0] = gqa_tensor(dk, sdk);
  a.dst[1] = gqa_tensor(dv, sdv);
  a.Sk = Sk;
  a.Hkv = Hkv;
  a.G = H / Hkv;
  a.per = (long)B * Sk * Hkv * kGqaChunks;
  const long need = (2 * a.per + kGqaThreads - 1) / kGqaThreads;
  long cap = (long)ljs_device_cus() * kGqaBlocksPerCu;
  if (g_gqa_max_blocks > 0) cap = g_gqa_max_blocks;
  const dim3 grid((unsigned)(need < cap ? need : cap));
  hipLaunchKernelGGL(gqa_reduce_kernel, grid, dim3(kGqaThreads), 0, st, a);
  ljs_launch_rec("gqa_reduce", grid, kGqaThreads);
  return (int)hipGetLastError();
}
