// Fused LayerNorm / RMSNorm over R rows of D contiguous features (row stride ld >= D), forward
// and backward in one launch each.
//
//   layer: xhat = (x - mu) r,  mu = mean(x),  r = 1 / sqrt(mean((x - mu)^2) + eps),  y = xhat g + b
//   rms:   xhat = x r,                        r = 1 / sqrt(mean(x^2) + eps),         y = xhat g
//
// x, y (and the backward's cotangent / dx) are f32 or bf16 independently; statistics and all
// arithmetic are f32.  A row lives in registers from its one read to its one write: the variance is
// the mean of the CENTRED squares (a second pass over registers), never E[x^2] - mu^2, which has no
// correct digit left once |mu| >> sigma; the mean itself is refined once by the mean of the
// centred values, which a single f32 sum around a large offset leaves measurably off.
//
// Two mappings of rows to threads, chosen by D alone (kWaveMaxD):
//   wave  (D <= 1024): one wave per row, lane l holds the 8-element chunks l, l + 64; the row sums
//         are 64-lane shuffles, no LDS.  D <= 512 takes two rows per wave at a time.
//   block (D  > 1024): one 256-thread block per row, thread t holds the chunks t, t + 256, ..;
//         the four waves' sums meet in 16 floats of LDS.
// The memory-bound loops move 16 bytes per lane per access.
//
// Backward: dx per row as above; d(gamma) = sum_rows g xhat and d(beta) = sum_rows g are kept per
// thread over the rows it visits, combined over the block's waves in wave order, written as one
// f32 partial row per block with write-through stores, and summed in block order by the last
// arriver of each group of 32 blocks, then in group order by the last group (the block form of
// rowwise.h's last-arriver hand-off).  No memset, no float atomics; the order of
// every sum is fixed by (R, D), so the result is the same bits on every run, and the tickets are
// zero again when the launch ends (a replayed graph finds them armed).
#include "rowwise.h"
#include <type_traits>

namespace {

constexpr int kWaveMaxD = 1024;     // widest row of the wave mapping
constexpr int kMaxD = 8192;
constexpr int kFwdWaves = 4;        // wave mapping: waves (= rows in flight) per forward block
constexpr int kBwdWaves = 8;        //               per backward block
constexpr int kFwdMaxBlocks = 2048;
constexpr int kBwdMaxBlocks = 512;  // = partial rows of the parameter gradients
constexpr int kTicketWords = 64;    // 1 + kBwdMaxBlocks / kTicketGroup, padded

// sums of a and b over the row: over the wave, or (BLOCK) over the block's four waves through
// red[2][4].  The caller gives every sum of a row its own red array and alternates between two
// sets from row to row, so a wave that is already writing a later sum cannot overtake one still
// reading this one (a barrier of the row between lies in between).
template <bool BLOCK>
__device__ __forceinline__ void row_sum2(float& a, float& b, float (*red)[4]) {
  a = warp_sum64(a);
  b = warp_sum64(b);
  if constexpr (BLOCK) {
    const int w = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) { red[0][w] = a; red[1][w] = b; }
    __syncthreads();
    a = (red[0][0] + red[0][1]) + (red[0][2] + red[0][3]);
    b = (red[1][0] + red[1][1]) + (red[1][2] + red[1][3]);
  }
}

// p[0] + p[n] + .. + p[(cnt - 1) n] in that order, B write-through loads in flight at a time: a
// chain of dependent reads of other blocks' partial rows costs a cross-XCD round trip each
template <int B>
__device__ __forceinline__ float partial_rows_step(const float*& p, unsigned& left, int n, float s) {
  while (left >= (unsigned)B) {
    float t[B];
#pragma unroll
    for (int k = 0; k < B; ++k) t[k] = sc1_load(p + (unsigned)(k * n));
#pragma unroll
    for (int k = 0; k < B; ++k) s += t[k];
    p += B * n;
    left -= B;
  }
  return s;
}
__device__ __forceinline__ float partial_rows_sum(const float* p, unsigned cnt, int n) {
  float s = partial_rows_step<16>(p, cnt, n, 0.f);
  s = partial_rows_step<4>(p, cnt, n, s);
  return partial_rows_step<1>(p, cnt, n, s);
}

template <bool LAYER, typename TX, typename TY, int NV, int U, bool BLOCK>
__global__ __launch_bounds__(BLOCK ? kRowBlockThreads : 64 * kFwdWaves)
void norm_fwd_kernel(const TX* __restrict__ x, long ldx, const float* __restrict__ gamma,
                     const float* __restrict__ beta, TY* __restrict__ y, long ldy, float* __restrict__ mean,
                     float* __restrict__ rstd, int R, int D, float eps) {
  static_assert(!BLOCK || U == 1, "the block mapping takes one row at a time");
  using M = RowMap<BLOCK, kFwdWaves>;
  __shared__ float red[2][3][2][4];  // [row parity][sum of the row][value][wave]
  const int slot = M::slot();
  const long step = M::step();
  const float inv_d = 1.f / (float)D;
  int col[NV];
  bool cv[NV];
  float gam[NV][8], bet[NV][8];
#pragma unroll
  for (int i = 0; i < NV; ++i) {
    col[i] = (i * M::W + slot) * 8;
    cv[i] = col[i] < D;
#pragma unroll
    for (int k = 0; k < 8; ++k) { gam[i][k] = 1.f; bet[i][k] = 0.f; }
    if (cv[i] && gamma) load_chunk8(gamma + col[i], gam[i]);
    if (cv[i] && beta) load_chunk8(beta + col[i], bet[i]);
  }
  int par = 0;
  for (long r0 = M::first(); r0 < R; r0 += step * U, par ^= 1) {
    float v[U][NV][8];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const long row = r0 + u * step;
#pragma unroll
      for (int i = 0; i < NV; ++i) {
        if (row < R && cv[i]) {
          load_chunk8(x + row * ldx + col[i], v[u][i]);
        } else {
#pragma unroll
          for (int k = 0; k < 8; ++k) v[u][i][k] = 0.f;
        }
      }
    }
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const long row = r0 + u * step;
      if (row >= R) break;  // uniform over the wave (block mapping: U == 1, never taken)
      float mu = 0.f, q = 0.f, unused = 0.f;
      if constexpr (LAYER) {
        // the mean in two steps: a first estimate, then the mean of what is left after taking it
        // off.  One f32 sum of D values around an offset is only good to a few ulps of D x offset
        // (100 +- 1.5 over 648 features: 1e-5 of the spread, ten times torch's own error); the
        // remainders are small, so their sum is exact to well below that.
#pragma unroll
        for (int step2 = 0; step2 < 2; ++step2) {
          float s = 0.f;
#pragma unroll
          for (int i = 0; i < NV; ++i) {
            float t = 0.f;
#pragma unroll
            for (int k = 0; k < 8; ++k) t += v[u][i][k];
            s += t;
          }
          row_sum2<BLOCK>(s, unused, red[par][step2]);
          const float m = s * inv_d;
          mu += m;
#pragma unroll
          for (int i = 0; i < NV; ++i)
            if (cv[i]) {
#pragma unroll
              for (int k = 0; k < 8; ++k) v[u][i][k] -= m;
            }
        }
      }
#pragma unroll
      for (int i = 0; i < NV; ++i) {
        float t = 0.f;
#pragma unroll
        for (int k = 0; k < 8; ++k) t += v[u][i][k] * v[u][i][k];
        q += t;
      }
      row_sum2<BLOCK>(q, unused, red[par][2]);
      const float r = 1.f / sqrtf(q * inv_d + eps);
#pragma unroll
      for (int i = 0; i < NV; ++i)
        if (cv[i]) {
          float o[8];
#pragma unroll
          for (int k = 0; k < 8; ++k) o[k] = v[u][i][k] * r * gam[i][k] + bet[i][k];
          store_chunk8(y + row * ldy + col[i], o);
        }
      if (slot == 0) {
        rstd[row] = r;
        if constexpr (LAYER) mean[row] = mu;
      }
    }
  }
}

template <bool LAYER, typename TX, typename TG, int NV, int U, bool BLOCK>
__global__ __launch_bounds__(BLOCK ? kRowBlockThreads : 64 * kBwdWaves)
void norm_bwd_kernel(const TX* __restrict__ x, long ldx, const TG* __restrict__ g, long ldg,
                     const float* __restrict__ gamma, const float* __restrict__ mean,
                     const float* __restrict__ rstd, TX* __restrict__ dx, long lddx, int R, int D,
                     unsigned* __restrict__ tickets, float* __restrict__ part, float* __restrict__ gpart,
                     float* __restrict__ dgamma, float* __restrict__ dbeta, int want_dx, int want_dp) {
  static_assert(!BLOCK || U == 1, "the block mapping takes one row at a time");
  using M = RowMap<BLOCK, kBwdWaves>;
  constexpr int NQ = LAYER ? 2 : 1;  // parameter-gradient rows: d(gamma), and d(beta) for layer
  __shared__ float red[2][2][4];
  __shared__ int last_s;
  const int slot = M::slot();
  const long step = M::step();
  const float inv_d = 1.f / (float)D;
  int col[NV];
  bool cv[NV];
  float gam[NV][8], dgam[NV][8], dbet[NV][8];
#pragma unroll
  for (int i = 0; i < NV; ++i) {
    col[i] = (i * M::W + slot) * 8;
    cv[i] = col[i] < D;
#pragma unroll
    for (int k = 0; k < 8; ++k) { gam[i][k] = 1.f; dgam[i][k] = 0.f; dbet[i][k] = 0.f; }
    if (cv[i] && gamma) load_chunk8(gamma + col[i], gam[i]);
  }
  int par = 0;
  for (long r0 = M::first(); r0 < R; r0 += step * U, par ^= 1) {
    float xv[U][NV][8], gv[U][NV][8];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const long row = r0 + u * step;
#pragma unroll
      for (int i = 0; i < NV; ++i) {
        if (row < R && cv[i]) {
          load_chunk8(x + row * ldx + col[i], xv[u][i]);
          load_chunk8(g + row * ldg + col[i], gv[u][i]);
        } else {
#pragma unroll
          for (int k = 0; k < 8; ++k) { xv[u][i][k] = 0.f; gv[u][i][k] = 0.f; }
        }
      }
    }
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const long row = r0 + u * step;
      if (row >= R) break;  // uniform over the wave (block mapping: U == 1, never taken)
      const float r = rstd[row];
      const float mu = LAYER ? mean[row] : 0.f;
      float s1 = 0.f, s2 = 0.f;
      // xv becomes xhat, gv stays g; a chunk past D holds g = 0, so it adds nothing anywhere
#pragma unroll
      for (int i = 0; i < NV; ++i) {
        float t1 = 0.f, t2 = 0.f;
#pragma unroll
        for (int k = 0; k < 8; ++k) {
          const float xh = (xv[u][i][k] - mu) * r;
          const float gy = gv[u][i][k] * gam[i][k];
          xv[u][i][k] = xh;
          t1 += gy;
          t2 += gy * xh;
          dgam[i][k] += gv[u][i][k] * xh;
          dbet[i][k] += gv[u][i][k];
        }
        s1 += t1;
        s2 += t2;
      }
      if (want_dx) {
        row_sum2<BLOCK>(s1, s2, red[par]);
        const float m1 = LAYER ? s1 * inv_d : 0.f, m2 = s2 * inv_d;
#pragma unroll
        for (int i = 0; i < NV; ++i)
          if (cv[i]) {
            float o[8];
#pragma unroll
            for (int k = 0; k < 8; ++k) o[k] = r * (gv[u][i][k] * gam[i][k] - m1 - xv[u][i][k] * m2);
            store_chunk8(dx + row * lddx + col[i], o);
          }
      }
    }
  }
  if (!want_dp) return;

  // ---- this block's partial row [NQ][D], written through
  float* mine = part + (long)blockIdx.x * NQ * D;
  if constexpr (BLOCK) {
    // every thread owns its columns
#pragma unroll
    for (int i = 0; i < NV; ++i)
      if (cv[i]) {
#pragma unroll
        for (int k = 0; k < 8; ++k) {
          sc1_store(mine + col[i] + k, dgam[i][k]);
          if constexpr (LAYER) sc1_store(mine + D + col[i] + k, dbet[i][k]);
        }
      }
  } else {
    // the waves hold the same columns: added up in LDS in wave order
    __shared__ float acc[NQ][kWaveMaxD];
    const int wave = threadIdx.x >> 6;
    for (int w = 0; w < kBwdWaves; ++w) {
      if (wave == w) {
#pragma unroll
        for (int i = 0; i < NV; ++i)
          if (cv[i]) {
#pragma unroll
            for (int k = 0; k < 8; ++k) {
              const int c = col[i] + k;
              acc[0][c] = w == 0 ? dgam[i][k] : acc[0][c] + dgam[i][k];
              if constexpr (LAYER) acc[1][c] = w == 0 ? dbet[i][k] : acc[1][c] + dbet[i][k];
            }
          }
      }
      __syncthreads();
    }
    for (int c = threadIdx.x; c < D; c += blockDim.x) {
      sc1_store(mine + c, acc[0][c]);
      if constexpr (LAYER) sc1_store(mine + D + c, acc[1][c]);
    }
  }
  const TicketGroup tg = ticket_group(blockIdx.x, gridDim.x);
  if (!block_last(tickets + 1 + tg.grp, tg.in_grp, &last_s)) return;

  // ---- last block of its group: the group's partial rows summed in block order
  const int n = NQ * D;
  const float* gbase = part + (long)tg.grp * kTicketGroup * n;
  for (int c = threadIdx.x; c < n; c += blockDim.x) {
    const float s = partial_rows_sum(gbase + c, tg.in_grp, n);
    sc1_store(gpart + (long)tg.grp * n + c, s);
  }
  if (!block_last(tickets, tg.ngrp, &last_s)) return;

  // ---- last group: the group sums in group order
  for (int c = threadIdx.x; c < n; c += blockDim.x) {
    const float s = partial_rows_sum(gpart + c, tg.ngrp, n);
    if (c < D) {
      if (dgamma) dgamma[c] = s;
    } else if (dbeta) {
      dbeta[c - D] = s;
    }
  }
}

// 0: wave, D <= 512, two rows per wave at a time; 1: wave, D <= 1024; 2: block
inline int norm_cfg(int D) { return D <= 512 ? 0 : (D <= kWaveMaxD ? 1 : 2); }

inline bool aligned16(const void* p, long ld, int elem) {
  return (((uintptr_t)p) & 15) == 0 && (ld * elem) % 16 == 0;
}

inline int fwd_grid(int R, int cfg) {
  const long per = cfg == 2 ? 1 : (long)kFwdWaves * (cfg == 0 ? 2 : 1);
  const long g = (R + per - 1) / per;
  return (int)(g < kFwdMaxBlocks ? g : kFwdMaxBlocks);
}
inline int bwd_grid(int R, int cfg) {
  const long per = cfg == 2 ? 1 : (long)kBwdWaves * (cfg == 0 ? 2 : 1);
  const long g = (R + per - 1) / per;
  return (int)(g < kBwdMaxBlocks ? g : kBwdMaxBlocks);
}

template <bool LAYER, typename TX, typename TY>
int launch_fwd(const char* wave_name, const char* block_name, const void* x, long ldx, const void* gamma,
               const void* beta, void* y, long ldy, void* mean, void* rstd, int R, int D, float eps,
               hipStream_t s) {
  const int cfg = norm_cfg(D);
  const dim3 grid(fwd_grid(R, cfg));
  const unsigned block = cfg == 2 ? kRowBlockThreads : 64 * kFwdWaves;
#define LJS_NORM_FWD(NV, U, BLOCK)                                                                              \
  hipLaunchKernelGGL((norm_fwd_kernel<LAYER, TX, TY, NV, U, BLOCK>), grid, dim3(block), 0, s, (const TX*)x, ldx, \
                     (const float*)gamma, (const float*)beta, (TY*)y, ldy, (float*)mean, (float*)rstd, R, D, eps)
  if (cfg == 0) LJS_NORM_FWD(1, 2, false);
  else if (cfg == 1) LJS_NORM_FWD(2, 1, false);
  else LJS_NORM_FWD(4, 1, true);
#undef LJS_NORM_FWD
  ljs_launch_rec(cfg == 2 ? block_name : wave_name, grid, block);
  return (int)hipGetLastError();
}

template <bool LAYER, typename TX, typename TG>
int launch_bwd(const char* wave_name, const char* block_name, const void* x, long ldx, const void* g, long ldg,
               const void* gamma, const void* mean, const void* rstd, void* dx, long lddx, int R, int D, void* ws,
               void* dgamma, void* dbeta, int want_dp, hipStream_t s) {
  const int cfg = norm_cfg(D);
  const int nb = bwd_grid(R, cfg);
  const dim3 grid(nb);
  const unsigned block = cfg == 2 ? kRowBlockThreads : 64 * kBwdWaves;
  const long n = (LAYER ? 2 : 1) * (long)D;
  unsigned* tickets = (unsigned*)ws;
  float* part = (float*)ws + kTicketWords;
  float* gpart = part + (long)nb * n;
#define LJS_NORM_BWD(NV, U, BLOCK)                                                                              \
  hipLaunchKernelGGL((norm_bwd_kernel<LAYER, TX, TG, NV, U, BLOCK>), grid, dim3(block), 0, s, (const TX*)x, ldx, \
                     (const TG*)g, ldg, (const float*)gamma, (const float*)mean, (const float*)rstd, (TX*)dx,    \
                     lddx, R, D, tickets, part, gpart, (float*)dgamma, (float*)dbeta, dx != nullptr ? 1 : 0,     \
                     want_dp)
  if (cfg == 0) LJS_NORM_BWD(1, 2, false);
  else if (cfg == 1) LJS_NORM_BWD(2, 1, false);
  else LJS_NORM_BWD(4, 1, true);
#undef LJS_NORM_BWD
  ljs_launch_rec(cfg == 2 ? block_name : wave_name, grid, block);
  return (int)hipGetLastError();
}

inline bool shape_ok(int R, int D) { return R >= 1 && D >= 8 && D <= kMaxD && D % 8 == 0; }

}  // namespace

// bytes of the backward's persistent workspace for R rows of D features: ticket words, one
// partial row per block, one per group of 32 blocks (zeroed once; the kernel re-arms the tickets)
LJS_API long ljs_norm_bwd_ws_bytes(int R, int D) {
  if (!shape_ok(R, D)) return 0;
  const long nb = bwd_grid(R, norm_cfg(D));
  const long ngrp = (nb + kTicketGroup - 1) / kTicketGroup;
  return 4 * (kTicketWords + (nb + ngrp) * 2L * D);
}

// kind: 0 = layer, 1 = rms.  gamma / beta may be null (1 / 0); mean is written for layer only.
LJS_API int ljs_norm_fwd(const void* x, int x_bf16, long ldx, const void* gamma, const void* beta, void* y,
                         int y_bf16, long ldy, void* mean, void* rstd, int R, int D, float eps, int kind,
                         hipStream_t s) {
  if (!shape_ok(R, D) || ldx < D || ldy < D || !x || !y || !rstd || (kind == 0 && !mean) || kind < 0 || kind > 1 ||
      !aligned16(x, ldx, x_bf16 ? 2 : 4) || !aligned16(y, ldy, y_bf16 ? 2 : 4) || !aligned16(gamma, 0, 4) ||
      !aligned16(beta, 0, 4))
    return (int)hipErrorInvalidValue;
#define LJS_NORM_CASE(LAYER, KS, TX, XS, TY, YS)                                                             \
  if ((kind == 0) == LAYER && (x_bf16 != 0) == std::is_same<TX, bf16_t>::value &&                            \
      (y_bf16 != 0) == std::is_same<TY, bf16_t>::value)                                                      \
    return launch_fwd<LAYER, TX, TY>("norm_fwd<" KS "," XS "," YS ",wave>", "norm_fwd<" KS "," XS "," YS     \
                                     ",block>", x, ldx, gamma, LAYER ? beta : nullptr, y, ldy, mean, rstd, R, \
                                     D, eps, s);
  LJS_NORM_CASE(true, "layer", float, "f32", float, "f32")
  LJS_NORM_CASE(true, "layer", float, "f32", bf16_t, "bf16")
  LJS_NORM_CASE(true, "layer", bf16_t, "bf16", float, "f32")
  LJS_NORM_CASE(true, "layer", bf16_t, "bf16", bf16_t, "bf16")
  LJS_NORM_CASE(false, "rms", float, "f32", float, "f32")
  LJS_NORM_CASE(false, "rms", float, "f32", bf16_t, "bf16")
  LJS_NORM_CASE(false, "rms", bf16_t, "bf16", float, "f32")
  LJS_NORM_CASE(false, "rms", bf16_t, "bf16", bf16_t, "bf16")
#undef LJS_NORM_CASE
  return (int)hipErrorInvalidValue;
}

// g: the cotangent of y (y's dtype); dx (x's dtype) may be null: not computed.  dgamma / dbeta
// (f32 [D]) may be null: with both null no parameter gradient is formed and ws is not touched,
// else ws holds >= ljs_norm_bwd_ws_bytes(R, D) bytes, zero at rest.
LJS_API int ljs_norm_bwd(const void* x, int x_bf16, long ldx, const void* g, int g_bf16, long ldg, const void* gamma,
                         const void* mean, const void* rstd, void* dx, long lddx, int R, int D, int kind, void* ws,
                         void* dgamma, void* dbeta, hipStream_t s) {
  const int want_dp = (dgamma || dbeta) ? 1 : 0;
  if (!shape_ok(R, D) || ldx < D || ldg < D || (dx && lddx < D) || !x || !g || !rstd || (kind == 0 && !mean) ||
      kind < 0 || kind > 1 || (want_dp && !ws) || (!dx && !want_dp) || !aligned16(x, ldx, x_bf16 ? 2 : 4) ||
      !aligned16(g, ldg, g_bf16 ? 2 : 4) || !aligned16(dx, dx ? lddx : 0, x_bf16 ? 2 : 4) ||
      !aligned16(gamma, 0, 4))
    return (int)hipErrorInvalidValue;
#define LJS_NORM_CASE(LAYER, KS, TX, XS, TG, GS)                                                             \
  if ((kind == 0) == LAYER && (x_bf16 != 0) == std::is_same<TX, bf16_t>::value &&                            \
      (g_bf16 != 0) == std::is_same<TG, bf16_t>::value)                                                      \
    return launch_bwd<LAYER, TX, TG>("norm_bwd<" KS "," XS "," GS ",wave>", "norm_bwd<" KS "," XS "," GS     \
                                     ",block>", x, ldx, g, ldg, gamma, mean, rstd, dx, lddx, R, D, ws,       \
                                     dgamma, LAYER ? dbeta : nullptr, want_dp, s);
  LJS_NORM_CASE(true, "layer", float, "f32", float, "f32")
  LJS_NORM_CASE(true, "layer", float, "f32", bf16_t, "bf16")
  LJS_NORM_CASE(true, "layer", bf16_t, "bf16", float, "f32")
  LJS_NORM_CASE(true, "layer", bf16_t, "bf16", bf16_t, "bf16")
  LJS_NORM_CASE(false, "rms", float, "f32", float, "f32")
  LJS_NORM_CASE(false, "rms", float, "f32", bf16_t, "bf16")
  LJS_NORM_CASE(false, "rms", bf16_t, "bf16", float, "f32")
  LJS_NORM_CASE(false, "rms", bf16_t, "bf16", bf16_t, "bf16")
#undef LJS_NORM_CASE
  return (int)hipErrorInvalidValue;
}
