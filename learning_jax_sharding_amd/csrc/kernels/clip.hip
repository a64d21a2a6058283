// Global-norm gradient clipping and learning-rate schedules inside the captured training step:
//   grad_sumsq  - multi-tensor sum of squares over the gradient-source table of the fused Adam,
//                 read where the gradients lie (plain f32 / bf16 tensors, split-K slabs summed in
//                 slab_reduce's order and then squared, constant gradients): no combine launch
//   step_hyper  - one wave: sum of the launches' (or the devices') float64 sums in index order,
//                 the norm, the clipping scale and the step's learning rate -> one StepHyper record
//                 that the dynamic Adam instance (elementwise.hip, adam_multi_kernel<.., true>) reads
#include "adam_common.h"
#include <algorithm>
#include <math.h>

namespace {

// ------------------------------------------------------------------ grad_sumsq
// Tiles of 32 rows x 64 columns (the Adam launch's default), one block of 256 threads per tile up
// to kSumsqMaxBlocks blocks, tiles dealt round-robin beyond that.  A thread squares and adds 8
// elements of each of its tiles in f32: 4 consecutive columns of 2 rows where the Adam 4-wide
// path's conditions hold for the gradient source (16-byte f32 / 8-byte bf16 loads), else one
// column of 8 rows (scalar loads: ragged or misaligned tensors).  Then a fixed tree: the 64-lane
// xor butterfly, the block's 4 wave sums added in wave order, one f32 partial per block written
// through (sc1), the two-level arrival ticket of rowwise.h; the last arriver adds the partials in
// block-index order in float64 and writes the launch's slot.  No float atomics, no memset; every
// ticket word is re-armed by the arriver that completed it (graph replay finds them zero).
constexpr int kSumsqRows = 32, kSumsqThreads = 256, kSumsqMaxBlocks = 1024, kSumsqSlots = 64;
// the workspace in 4-byte words: one f32 partial per block, the ticket words, the float64 slots
constexpr int kSumsqTicketWord = kSumsqMaxBlocks;
constexpr int kSumsqSlotWord = kSumsqTicketWord + 64;   // (1 + 1024 / 32 = 33 ticket words, padded)
constexpr int kSumsqWsWords = kSumsqSlotWord + 2 * kSumsqSlots;
static_assert(1 + kSumsqMaxBlocks / (int)kTicketGroup <= 64 && kSumsqSlotWord % 2 == 0, "workspace layout");

struct SumsqBatch {
  AdamTensor t[kAdamMax];
  int tile_start[kAdamMax + 1];
  int n;
};

__device__ __forceinline__ void add_sq4(float& acc, const f32x4& g) {
#pragma unroll
  for (int e = 0; e < 4; ++e) acc += g[e] * g[e];
}

__global__ __launch_bounds__(kSumsqThreads) void grad_sumsq_kernel(SumsqBatch batch, float* __restrict__ partials,
                                                                    unsigned* __restrict__ tickets,
                                                                    double* __restrict__ slot) {
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int c4 = (threadIdx.x & 15) * 4, r0 = threadIdx.x >> 4;
  const int total = batch.tile_start[batch.n];
  float acc = 0.f;
  for (int id = blockIdx.x; id < total; id += gridDim.x) {
    int ti = 0;
#pragma unroll
    for (int i = 1; i < kAdamMax; ++i) ti += (i < batch.n && id >= batch.tile_start[i]) ? 1 : 0;
    const AdamTensor& T = batch.t[ti];
    const long R = T.R, C = T.C, gS = T.gS, g_ld = T.g_ld, g_ss = T.g_ss;
    const bool bf = T.g_bf16 != 0;
    const int local = id - batch.tile_start[ti];
    const int tr_i = local / (int)T.tiles_c, tc_i = local % (int)T.tiles_c;
    if (gS >= 0 && T.vec && (long)(tc_i + 1) * 64 <= C) {
      const long cbase = (long)tc_i * 64 + c4;
      f32x4 g[2];
      bool ok[2];
#pragma unroll
      for (int q = 0; q < 2; ++q) {
        const long row = (long)tr_i * kSumsqRows + r0 + 16 * q;
        ok[q] = row < R;
        const long gi = (ok[q] ? row : 0) * g_ld + cbase;   // (a row past the end re-reads row 0, unused)
        if (gS > 0) {
          g[q] = bf ? slab_sum4(reinterpret_cast<const bf16_t*>(T.g), gS, g_ss, gi)
                    : slab_sum4(reinterpret_cast<const float*>(T.g), gS, g_ss, gi);
        } else {
          g[q] = bf ? ld_slab4(reinterpret_cast<const bf16_t*>(T.g), gi)
                    : ld_slab4(reinterpret_cast<const float*>(T.g), gi);
        }
      }
#pragma unroll
      for (int q = 0; q < 2; ++q)
        if (ok[q]) add_sq4(acc, g[q]);
      continue;
    }
    const long col = (long)tc_i * 64 + lane;
#pragma unroll 4
    for (int rr = 0; rr < kSumsqRows / 4; ++rr) {
      const long row = (long)tr_i * kSumsqRows + w + 4 * rr;
      if (row < R && col < C) {
        const long gi = row * g_ld + col;
        const float g = gS > 0   ? (bf ? slab_sum1(reinterpret_cast<const bf16_t*>(T.g), gS, g_ss, gi)
                                       : slab_sum1(reinterpret_cast<const float*>(T.g), gS, g_ss, gi))
                        : gS < 0 ? __int_as_float((int)g_ld)
                        : bf     ? bf2f(reinterpret_cast<const bf16_t*>(T.g)[gi])
                                 : reinterpret_cast<const float*>(T.g)[gi];
        acc += g * g;
      }
    }
  }
  acc = warp_sum64(acc);
  __shared__ float part[kSumsqThreads / 64];
  if (lane == 0) part[w] = acc;
  __syncthreads();
  if (w != 0) return;
  if (lane == 0) {
    float t = part[0];
#pragma unroll
    for (int k = 1; k < kSumsqThreads / 64; ++k) t += part[k];
    sc1_store(partials + blockIdx.x, t);
  }
  if (!wave_last_2lvl(tickets, blockIdx.x, gridDim.x)) return;
  // the last arriver: every block's partial is in memory; added in block-index order in float64
  // Every load is issued before the first add (one round trip, not one per 64 partials) and parked
  // in LDS; a round of 64 is then folded with constant-lane v_readlane, so the only serial chain is
  // the float64 adds, in a loop body of one round (a looped __shfl cost ~35 us for 660 blocks, the
  // fold unrolled over all 16 rounds ~10 us of cold instruction fetch).  A missing block adds +0.
  constexpr int kRounds = kSumsqMaxBlocks / 64;
  __shared__ float parked[kSumsqMaxBlocks];
  float v[kRounds];
#pragma unroll
  for (int r = 0; r < kRounds; ++r) {
    const unsigned i = r * 64 + lane;
    v[r] = i < gridDim.x ? sc1_load(partials + i) : 0.f;
  }
#pragma unroll
  for (int r = 0; r < kRounds; ++r) parked[r * 64 + lane] = v[r];   // (this wave only: no barrier)
  double sum = 0.0;
#pragma unroll 1
  for (unsigned r = 0; r * 64 < gridDim.x; ++r) {
    const unsigned x = __float_as_uint(parked[r * 64 + lane]);
#pragma unroll
    for (int l = 0; l < 64; ++l) sum += (double)__uint_as_float(__builtin_amdgcn_readlane(x, l));
  }
  if (lane == 0) *slot = sum;
}

// ------------------------------------------------------------------ step_hyper
// the optax formulas in float64 (optim/schedule.py evaluates the same ones on the host)
struct SchedArgs {
  int kind;       // 0 constant, 1 linear, 2 cosine decay, 3 warmup + cosine decay
  double p[5];    // optim/schedule.py Schedule.params
};
__device__ __forceinline__ double sched_linear(double init, double end, double steps, double begin, double count) {
  if (steps <= 0.0) return init;
  const double c = fmin(fmax(count - begin, 0.0), steps);
  return (init - end) * (1.0 - c / steps) + end;
}
__device__ __forceinline__ double sched_cosine(double init, double decay_steps, double alpha, double count) {
  const double c = fmin(count, decay_steps);
  return init * ((1.0 - alpha) * 0.5 * (1.0 + cos(M_PI * c / decay_steps)) + alpha);
}
__device__ __forceinline__ double sched_value(const SchedArgs& s, double count) {
  switch (s.kind) {
    case 1: return sched_linear(s.p[0], s.p[1], s.p[2], s.p[3], count);
    case 2: return sched_cosine(s.p[0], s.p[1], s.p[2], count);
    case 3: return count < s.p[2] ? sched_linear(s.p[0], s.p[1], s.p[2], 0.0, count)
                                  : sched_cosine(s.p[1], s.p[3], s.p[4], count - s.p[2]);
    default: return s.p[0];
  }
}

// One wave (every lane computes the same values; lane 0 stores).  sumsq = the n_slots launch slots
// added in index order, or, when `gathered` is given, the n_gathered per-device sums in device-id
// order (every device adds the same vector in the same order: the same bits everywhere).
// partial_out != null: only write the slots' sum there (a device's contribution to the gather).
// The count the schedule sees is *step + step_offset - 1: step_offset follows ljs_adam_multi
// (t = *step + step_offset is the step being taken, counted from 1).
__global__ __launch_bounds__(64) void step_hyper_kernel(const double* __restrict__ slots, int n_slots,
                                                        const double* __restrict__ gathered, int n_gathered,
                                                        double* __restrict__ partial_out, const int* __restrict__ step,
                                                        int step_offset, int clip, double max_norm, SchedArgs sched,
                                                        StepHyper* __restrict__ rec) {
  double s = 0.0;
  for (int i = 0; i < n_slots; ++i) s += slots[i];
  if (partial_out) {
    if (threadIdx.x == 0) *partial_out = s;
    return;
  }
  if (gathered) {
    s = 0.0;
    for (int i = 0; i < n_gathered; ++i) s += gathered[i];
  }
  const double norm = sqrt(s);
  const double scale = (!clip || norm < max_norm) ? 1.0 : max_norm / norm;
  const double count = (double)(*step + step_offset - 1);
  const double lr = sched_value(sched, count);
  if (threadIdx.x == 0) {
    rec->grad_scale = (float)scale;
    rec->lr = (float)lr;
    rec->norm = (float)norm;
    rec->pad = 0.f;
  }
}

}  // namespace

LJS_API long ljs_grad_sumsq_ws_words() { return kSumsqWsWords; }
LJS_API long ljs_grad_sumsq_slot_word() { return kSumsqSlotWord; }
LJS_API long ljs_grad_sumsq_slots() { return kSumsqSlots; }

// table: the n x 16 int64 rows of ljs_adam_multi (only the shape and the gradient source are
// read); ws: the persistent zero-initialised workspace of ljs_grad_sumsq_ws_words() words; the
// launch's float64 sum goes to slot `slot` of the workspace
LJS_API int ljs_grad_sumsq(const long* table, int n, void* ws, int slot, hipStream_t s) {
  if (n < 1 || n > kAdamMax || slot < 0 || slot >= kSumsqSlots || !ws || ((uintptr_t)ws & 7))
    return (int)hipErrorInvalidValue;
  SumsqBatch b;
  long tiles = 0;
  for (int i = 0; i < n; ++i) {
    AdamTensor& t = b.t[i];
    t = AdamTensor{};
    if (!adam_grad_from_row(table + 16 * i, t)) return (int)hipErrorInvalidValue;
    if (t.R < 0 || t.C < 0 || (t.gS >= 0 && !t.g && t.R * t.C > 0)) return (int)hipErrorInvalidValue;
    t.vec = adam_grad_vec_ok(t);
    b.tile_start[i] = (int)tiles;
    tiles += ((t.R + kSumsqRows - 1) / kSumsqRows) * t.tiles_c;
    if (tiles > 0x7fffffffL) return (int)hipErrorInvalidValue;
  }
  b.tile_start[n] = (int)tiles;
  b.n = n;
  const unsigned grid = (unsigned)std::max<long>(1, std::min<long>(tiles, kSumsqMaxBlocks));
  float* partials = (float*)ws;
  ljs_launch_rec("grad_sumsq", dim3(grid), kSumsqThreads);
  hipLaunchKernelGGL(grad_sumsq_kernel, dim3(grid), dim3(kSumsqThreads), 0, s, b, partials,
                     (unsigned*)ws + kSumsqTicketWord, (double*)((unsigned*)ws + kSumsqSlotWord) + slot);
  return (int)hipGetLastError();
}

// slots / gathered / partial_out: see step_hyper_kernel.  clip = 0: no clipping (grad_scale = 1;
// the norm is that of whatever sums were given, 0 for none).  rec: 16 bytes, 16-byte aligned.
LJS_API int ljs_step_hyper(const void* slots, int n_slots, const void* gathered, int n_gathered, void* partial_out,
                           const void* step, int step_offset, int clip, double max_norm, int kind, double p0,
                           double p1, double p2, double p3, double p4, void* rec, hipStream_t s) {
  if (n_slots < 0 || n_slots > kSumsqSlots || (n_slots > 0 && !slots) || n_gathered < 0 || (gathered && n_gathered < 1))
    return (int)hipErrorInvalidValue;
  if (!partial_out && (!rec || ((uintptr_t)rec & 15) || !step || kind < 0 || kind > 3)) return (int)hipErrorInvalidValue;
  SchedArgs sa{kind, {p0, p1, p2, p3, p4}};
  ljs_launch_rec("step_hyper", dim3(1), 64);
  hipLaunchKernelGGL(step_hyper_kernel, dim3(1), dim3(64), 0, s, (const double*)slots, n_slots, (const double*)gathered,
                     gathered ? n_gathered : 0, (double*)partial_out, (const int*)step, step_offset, clip, max_norm, sa,
                     (StepHyper*)rec);
  return (int)hipGetLastError();
}
