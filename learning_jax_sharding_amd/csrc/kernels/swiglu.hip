// Fused SwiGLU activation of a gated feed-forward: h = silu(g) u forward, (dg, du) backward.
//
// With sigma the logistic function and c = 1 - sigma:
//
//     h  = g sigma(g) u
//     du = dh sigma(g) g
//     dg = dh sigma(g) u (1 + g c(g))
//
// The backward recomputes sigma from g: nothing is saved besides g and u, which the gate / up and
// down projections keep anyway.  All arithmetic is f32 with one rounding to the output dtype.
//
// sigma and c come from ONE exp2 of a non-positive argument, so nothing overflows for any finite g:
//
//     e = exp2(-|g| log2e),  r = 1 / (1 + e),   sigma = g >= 0 ? r : e r,   c = g >= 0 ? e r : r
//
// c is never formed as 1 - sigma (that subtraction loses c below one ulp of 1, g above about 16).
// The instruction sequence per element, which tests/swiglu_oracle.py derives its bounds from:
// v_mul (the argument), v_exp_f32, v_add, v_rcp_f32, v_mul (e r), then forward v_mul (g sigma),
// v_mul (u); backward v_mul (dh sigma), v_mul (g) for du, v_mul (u), v_fma (1 + g c), v_mul for dg.
//
// Tensors are (B, S, F) with F contiguous and their own batch / position strides (in elements):
// the two column blocks of the fused [T][2 F] gate / up projection buffer and seq-major storage
// are read and written in place.  F is a multiple of 8 with no upper bound; every base and stride
// is 16-byte aligned; offsets are 64-bit.  g, u, dg, du share one dtype and h, dh another, f32 or
// bf16 each.
//
// One work item is (batch, position, group j): the G features [j G, j G + G), G = 8 when a bf16
// side is involved (one bf16 chunk, two f32 chunks) and 4 for f32 -> f32.  No LDS, no cross-lane
// traffic, no atomics, no workspace.  Items are taken grid-stride; the group index runs fastest,
// so a wave reads and writes whole contiguous row segments.
#include "rowwise.h"
#include <type_traits>

namespace {

constexpr int kSwigluThreads = kRowBlockThreads;
constexpr int kSwigluBlocksPerCu = 8;   // 8 blocks x 4 waves: every wave slot of a CU
constexpr float kSwigluLog2e = 1.44269504088896340736f;

int g_swiglu_max_blocks = 0;            // > 0: a grid cap for tests (grid-stride on small shapes)

struct SwigluTensor {
  void* p;
  long sb, ss;                          // strides (elements): batch, position
};

struct SwigluArgs {
  SwigluTensor g, u, h;                 // h: the forward's output, the backward's cotangent dh
  SwigluTensor dg, du;                  // backward only
  long total;                           // items: B S (F / G)
  int S, ng;                            // positions per batch, groups per row
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

// sigma(g) and c = 1 - sigma(g), see the head of the file
__device__ __forceinline__ void sigmoid_pair(float g, float& sg, float& c) {
  const float e = __builtin_amdgcn_exp2f(-fabsf(g) * kSwigluLog2e);
  const float r = __builtin_amdgcn_rcpf(1.0f + e);
  const float er = e * r;
  sg = g >= 0.0f ? r : er;
  c = g >= 0.0f ? er : r;
}

template <typename T>
__device__ __forceinline__ T* at(const SwigluTensor& t, long b, int s, int j, int G) {
  return (T*)t.p + b * t.sb + (long)s * t.ss + (long)j * G;
}

// TI: g, u (and dg, du); TO: h (and dh)
template <typename TI, typename TO, bool BWD>
__global__ __launch_bounds__(kSwigluThreads)
void swiglu_kernel(const SwigluArgs a) {
  constexpr int G = (sizeof(TI) == 2 || sizeof(TO) == 2) ? 8 : 4;
  const long step = (long)gridDim.x * kSwigluThreads;
  for (long item = (long)blockIdx.x * kSwigluThreads + threadIdx.x; item < a.total; item += step) {
    const int j = (int)(item % a.ng);
    const long r = item / a.ng;
    const int s = (int)(r % a.S);
    const long b = r / a.S;
    float g[G], u[G];
    load_group<G>(at<const TI>(a.g, b, s, j, G), g);
    load_group<G>(at<const TI>(a.u, b, s, j, G), u);
    if constexpr (!BWD) {
      float h[G];
#pragma unroll
      for (int e = 0; e < G; ++e) {
        float sg, c;
        sigmoid_pair(g[e], sg, c);
        h[e] = g[e] * sg * u[e];
      }
      store_group<G>(at<TO>(a.h, b, s, j, G), h);
    } else {
      float dh[G], dg[G], du[G];
      load_group<G>(at<const TO>(a.h, b, s, j, G), dh);
#pragma unroll
      for (int e = 0; e < G; ++e) {
        float sg, c;
        sigmoid_pair(g[e], sg, c);
        const float ds = dh[e] * sg;
        du[e] = ds * g[e];
        dg[e] = ds * u[e] * fmaf(g[e], c, 1.0f);
      }
      store_group<G>(at<TI>(a.dg, b, s, j, G), dg);
      store_group<G>(at<TI>(a.du, b, s, j, G), du);
    }
  }
}

inline bool swiglu_aligned(const void* p, const long* st, int elem) {
  return p && st && (((uintptr_t)p) & 15u) == 0 && (st[0] * elem) % 16 == 0 && (st[1] * elem) % 16 == 0;
}

template <typename TI, typename TO, bool BWD>
int swiglu_launch(const char* name, const SwigluArgs& a, hipStream_t st) {
  const long need = (a.total + kSwigluThreads - 1) / kSwigluThreads;
  long cap = (long)ljs_device_cus() * kSwigluBlocksPerCu;
  if (g_swiglu_max_blocks > 0) cap = g_swiglu_max_blocks;
  const dim3 grid((unsigned)(need < cap ? need : cap));
  hipLaunchKernelGGL((swiglu_kernel<TI, TO, BWD>), grid, dim3(kSwigluThreads), 0, st, a);
  ljs_launch_rec(name, grid, kSwigluThreads);
  return (int)hipGetLastError();
}

inline SwigluTensor swiglu_tensor(const void* p, const long* st) {
  return SwigluTensor{const_cast<void*>(p), st[0], st[1]};
}

template <bool BWD>
int swiglu_dispatch(SwigluArgs& a, int in_bf16, int out_bf16, int B, int S, int F, hipStream_t st) {
  if (B < 1 || S < 1 || F < 8 || F % 8 != 0) return (int)hipErrorInvalidValue;
  const int G = (in_bf16 || out_bf16) ? 8 : 4;
  a.S = S;
  a.ng = F / G;
  a.total = (long)B * S * a.ng;
#define LJS_SWIGLU_CASE(TI, IS, TO, OS)                                                                    \
  if ((in_bf16 != 0) == std::is_same<TI, bf16_t>::value && (out_bf16 != 0) == std::is_same<TO, bf16_t>::value) \
    return BWD ? swiglu_launch<TI, TO, BWD>("swiglu_bwd<" OS "," IS ">", a, st)                            \
               : swiglu_launch<TI, TO, BWD>("swiglu<" IS "," OS ">", a, st);
  LJS_SWIGLU_CASE(float, "f32", float, "f32")
  LJS_SWIGLU_CASE(float, "f32", bf16_t, "bf16")
  LJS_SWIGLU_CASE(bf16_t, "bf16", float, "f32")
  LJS_SWIGLU_CASE(bf16_t, "bf16", bf16_t, "bf16")
#undef LJS_SWIGLU_CASE
  return (int)hipErrorInvalidValue;
}

}  // namespace

// tests: at most n blocks per launch (the grid-stride loop on small shapes); n <= 0: the default,
// kSwigluBlocksPerCu blocks per compute unit
LJS_API int ljs_swiglu_set_max_blocks(int n) {
  g_swiglu_max_blocks = n > 0 ? n : 0;
  return 0;
}

// g, u -> h = silu(g) u, all (B, S, F) with the strides sg / su / sh = (batch, position) in elements
// and F contiguous; g and u are f32 or bf16 by in_bf16, h by out_bf16.  Returns non-zero, and
// launches nothing, for an F that is not a multiple of 8 or a misaligned base or stride.
LJS_API int ljs_swiglu(const void* g, const void* u, void* h, int in_bf16, int out_bf16, int B, int S, int F,
                       const long* sg, const long* su, const long* sh, hipStream_t st) {
  const int ie = in_bf16 ? 2 : 4, oe = out_bf16 ? 2 : 4;
  if (!swiglu_aligned(g, sg, ie) || !swiglu_aligned(u, su, ie) || !swiglu_aligned(h, sh, oe))
    return (int)hipErrorInvalidValue;
  SwigluArgs a{};
  a.g = swiglu_tensor(g, sg);
  a.u = swiglu_tensor(u, su);
  a.h = swiglu_tensor(h, sh);
  return swiglu_dispatch<false>(a, in_bf16, out_bf16, B, S, F, st);
}

// g, u, dh -> dg, du (the dtype of g and u), recomputing sigma(g); dh has h's dtype (out_bf16).
// The same layout rules and return code as ljs_swiglu.
LJS_API int ljs_swiglu_bwd(const void* g, const void* u, const void* dh, void* dg, void* du, int in_bf16,
                           int out_bf16, int B, int S, int F, const long* sg, const long* su, const long* sdh,
                           const long* sdg, const long* sdu, hipStream_t st) {
  const int ie = in_bf16 ? 2 : 4, oe = out_bf16 ? 2 : 4;
  if (!swiglu_aligned(g, sg, ie) || !swiglu_aligned(u, su, ie) || !swiglu_aligned(dh, sdh, oe) ||
      !swiglu_aligned(dg, sdg, ie) || !swiglu_aligned(du, sdu, ie))
    return (int)hipErrorInvalidValue;
  SwigluArgs a{};
  a.g = swiglu_tensor(g, sg);
  a.u = swiglu_tensor(u, su);
  a.h = swiglu_tensor(dh, sdh);
  a.dg = swiglu_tensor(dg, sdg);
  a.du = swiglu_tensor(du, sdu);
  return swiglu_dispatch<true>(a, in_bf16, out_bf16, B, S, F, st);
}
