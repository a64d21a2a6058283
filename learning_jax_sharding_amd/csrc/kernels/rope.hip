// Fused rotary position embedding (RoPE) of Q and K in one launch, forward and inverse.
//
// Convention: half-split pairs (MaxText, Llama-HF).  For a head vector x[0:D] at global position p,
// with h = D / 2 and i in [0, h):
//
//     ang      = p * theta^(-2 i / D)
//     y[i]     = x[i]     cos(ang) - x[i + h] sin(ang)
//     y[i + h] = x[i + h] cos(ang) + x[i]     sin(ang)
//
// The inverse (the backward: dx = R(-ang) dy) is the same map with sin negated.  cos and sin come
// from a table the host computed in float64 and rounded once to f32, [P][h] each; nothing here
// evaluates sincos (in f32 the product p * inv_freq alone is off by about p * 2^-24 radians).
//
// Tensors are (B, S, H, D) with D contiguous and arbitrary batch / sequence / head strides (in
// elements), separately for q, k, q_out and k_out: column blocks of a fused [T][3 H D] projection
// buffer and seq-major storage are taken as they are.  Input and output are f32 or bf16
// independently, arithmetic in f32.  D is a multiple of 16 in 16..256, so each half is whole
// 16-byte chunks in both dtypes; every base and stride is 16-byte aligned; offsets are 64-bit.
//
// One work item is (tensor, batch, position, head, group j): the G elements [j G, j G + G) of the
// first half and the same elements of the second half, G = 8 when a bf16 side is involved (one bf16
// chunk, two f32 chunks) and 4 for f32 -> f32.  A lane loads its two groups and the matching cos /
// sin groups (the table stays in L2: S h 8 bytes), rotates in registers and writes two groups.  No
// LDS, no cross-lane traffic, no atomics, no workspace.  Items are taken grid-stride; the group
// index runs fastest, then the head, so a wave reads and writes whole contiguous rows.
#include "rowwise.h"
#include <type_traits>

namespace {

constexpr int kRopeThreads = kRowBlockThreads;
constexpr int kRopeBlocksPerCu = 8;   // 8 blocks x 4 waves: every wave slot of a CU
constexpr int kRopeMinD = 16, kRopeMaxD = 256;

int g_rope_max_blocks = 0;            // > 0: a grid cap for tests (grid-stride on small shapes)

struct RopeTensor {
  const void* in;
  void* out;
  long ib, is, ih;                    // input strides (elements): batch, position, head
  long ob, os, oh;                    // output strides
};

struct RopeArgs {
  RopeTensor t[2];
  const float* cos_t;
  const float* sin_t;
  long per_tensor;                    // items of one tensor: B S H (h / G)
  long total;                         // per_tensor x tensors
  long pos_offset;
  int S, H, h;
};

template <int G, typename T>
__device__ __forceinline__ void load_group(const T* p, float (&v)[G]) {
#pragma unroll
  for (int e = 0; e < G; e += 16 / (int)sizeof(T)) load_chunk(p + e, v + e);
}
template <int G, typename T>
__device__ __forceinline__ void store_group(T* p, const float (&v)[G]) {
#pragma unroll
  for (int e = 0; e < G; e += 16 / (int)sizeof(T)) store_chunk(p + e, v + e);
}

template <typename TI, typename TO, bool INV>
__global__ __launch_bounds__(kRopeThreads)
void rope_kernel(const RopeArgs a) {
  constexpr int G = (sizeof(TI) == 2 || sizeof(TO) == 2) ? 8 : 4;
  const int ng = a.h / G;             // groups per half
  const long step = (long)gridDim.x * kRopeThreads;
  for (long item = (long)blockIdx.x * kRopeThreads + threadIdx.x; item < a.total; item += step) {
    const int which = item >= a.per_tensor ? 1 : 0;
    long r = item - (which ? a.per_tensor : 0);
    const int j = (int)(r % ng);
    r /= ng;
    const int hd = (int)(r % a.H);
    r /= a.H;
    const int s = (int)(r % a.S);
    const long b = r / a.S;
    const RopeTensor& t = a.t[which];
    const TI* src = (const TI*)t.in + b * t.ib + (long)s * t.is + (long)hd * t.ih + j * G;
    TO* dst = (TO*)t.out + b * t.ob + (long)s * t.os + (long)hd * t.oh + j * G;
    const long trow = (a.pos_offset + s) * (long)a.h + j * G;
    float x0[G], x1[G], c[G], sn[G], y0[G], y1[G];
    load_group<G>(src, x0);
    load_group<G>(src + a.h, x1);
    load_group<G>(a.cos_t + trow, c);
    load_group<G>(a.sin_t + trow, sn);
#pragma unroll
    for (int e = 0; e < G; ++e) {
      const float sg = INV ? -sn[e] : sn[e];
      y0[e] = x0[e] * c[e] - x1[e] * sg;
      y1[e] = x1[e] * c[e] + x0[e] * sg;
    }
    store_group<G>(dst, y0);
    store_group<G>(dst + a.h, y1);
  }
}

inline bool rope_aligned(const void* p, const long* st, int elem) {
  return (((uintptr_t)p) & 15u) == 0 && (st[0] * elem) % 16 == 0 && (st[1] * elem) % 16 == 0 &&
         (st[2] * elem) % 16 == 0;
}

template <typename TI, typename TO, bool INV>
int rope_launch(const char* name, const RopeArgs& a, hipStream_t st) {
  const long need = (a.total + kRopeThreads - 1) / kRopeThreads;
  long cap = (long)ljs_device_cus() * kRopeBlocksPerCu;
  if (g_rope_max_blocks > 0) cap = g_rope_max_blocks;
  const dim3 grid((unsigned)(need < cap ? need : cap));
  hipLaunchKernelGGL((rope_kernel<TI, TO, INV>), grid, dim3(kRopeThreads), 0, st, a);
  ljs_launch_rec(name, grid, kRopeThreads);
  return (int)hipGetLastError();
}

}  // namespace

// tests: at most n blocks per launch (the grid-stride loop on small shapes); n <= 0: the default,
// kRopeBlocksPerCu blocks per compute unit
LJS_API int ljs_rope_set_max_blocks(int n) {
  g_rope_max_blocks = n > 0 ? n : 0;
  return 0;
}

// q, k -> q_out, k_out, all (B, S, H, D) with the strides sq / sk / sqo / sko = (batch, position,
// head) in elements and D contiguous; k and k_out may both be null: one tensor.  cos_t / sin_t:
// f32 [table_rows][D / 2]; the row of position s is pos_offset + s.  inverse != 0 rotates by -ang.
// Returns non-zero, and launches nothing, for an unsupported D or dtype pairing, a misaligned base
// or stride, or positions outside the table.
LJS_API int ljs_rope(const void* q, const void* k, void* q_out, void* k_out, int in_bf16, int out_bf16, int B, int S,
                     int H, int D, const long* sq, const long* sk, const long* sqo, const long* sko,
                     const void* cos_t, const void* sin_t, long table_rows, long pos_offset, int inverse,
                     hipStream_t st) {
  const int ie = in_bf16 ? 2 : 4, oe = out_bf16 ? 2 : 4;
  if (!q || !q_out || !sq || !sqo || (k == nullptr) != (k_out == nullptr) || (k && (!sk || !sko)) || !cos_t ||
      !sin_t || B < 1 || S < 1 || H < 1 || D < kRopeMinD || D > kRopeMaxD || D % 16 != 0 || pos_offset < 0 ||
      pos_offset + S > table_rows || (((uintptr_t)cos_t) & 15u) || (((uintptr_t)sin_t) & 15u) ||
      !rope_aligned(q, sq, ie) || !rope_aligned(q_out, sqo, oe) || (k && !rope_aligned(k, sk, ie)) ||
      (k && !rope_aligned(k_out, sko, oe)))
    return (int)hipErrorInvalidValue;
  RopeArgs a;
  a.t[0] = RopeTensor{q, q_out, sq[0], sq[1], sq[2], sqo[0], sqo[1], sqo[2]};
  a.t[1] = k ? RopeTensor{k, k_out, sk[0], sk[1], sk[2], sko[0], sko[1], sko[2]} : a.t[0];
  a.cos_t = (const float*)cos_t;
  a.sin_t = (const float*)sin_t;
  a.S = S;
  a.H = H;
  a.h = D / 2;
  a.pos_offset = pos_offset;
  const int G = (in_bf16 || out_bf16) ? 8 : 4;
  a.per_tensor = (long)B * S * H * (a.h / G);
  a.total = a.per_tensor * (k ? 2 : 1);
#define LJS_ROPE_CASE(TI, IS, TO, OS)                                                                    \
  if ((in_bf16 != 0) == std::is_same<TI, bf16_t>::value && (out_bf16 != 0) == std::is_same<TO, bf16_t>::value) \
    return inverse ? rope_launch<TI, TO, true>("rope<" IS "," OS ",inv>", a, st)                          \
                   : rope_launch<TI, TO, false>("rope<" IS "," OS ">", a, st);
  LJS_ROPE_CASE(float, "f32", float, "f32")
  LJS_ROPE_CASE(float, "f32", bf16_t, "bf16")
  LJS_ROPE_CASE(bf16_t, "bf16", float, "f32")
  LJS_ROPE_CASE(bf16_t, "bf16", bf16_t, "bf16")
#undef LJS_ROPE_CASE
  return (int)hipErrorInvalidValue;
}
