// The generic release/consider env over Nakamoto as lockstep lanes for gfx950
// (CPR_PROTO_GENERIC_NAKAMOTO, generic_lane.h):
//   k_generic_reset / _step   one thread per lane: the lane's 128-byte header is loaded into
//                             registers, stepped, and stored back as a unit; the block DAG
//                             stays in the lane's region of the batch's pool
//   k_generic_observe_fields, k_generic_cursor   seven fields per lane, the LaneCursor
//
// The pool is one allocation: n headers (one 128-byte line each), then n regions of
// generic_region_bytes(max_steps) bytes (whole lines), so no header shares a line with any
// block array. A lane's accesses to its region are its own: one thread per lane walks parent
// pointers and shifts list entries, lanes of a wave touch different lines, and the step is
// bound by those dependent loads, not by arithmetic (DESIGN.md §4.10a has the measurements).
// Every index the kernels form is below max_steps + 1: a block is added only while
// n_blocks <= max_steps (generic_step), and the lists hold distinct block indices.
#include <hip/hip_runtime.h>

#include "../../include/cpr_hip.h"
#include "generic_lane.h"
#include "kernels.h"
#include "summary.h"

#pragma clang fp contract(off)

namespace cpr {

using generic::GenericBlocks;
using generic::GenericLane;
using generic::GenericParams;

static_assert(sizeof(GenericLane) == 128, "the lane header is one 128-byte line");

struct GenericPool {
  GenericLane* lanes;  // [n]
  uint8_t* regions;    // [n][region]
  size_t region;
};

__device__ inline GenericBlocks lane_blocks(const GenericPool& M, const GenericParams& P,
                                            int64_t i) {
  return generic::generic_blocks(M.regions + (size_t)i * M.region, P.max_steps);
}

// the five f32 of the reference, widened into the f64 observation buffer
__device__ inline void lane_observe(const GenericBlocks& B, GenericLane& L, double* obs) {
  float o[5];
  generic::generic_observe(B, L, o);
  for (int k = 0; k < 5; ++k) obs[k] = (double)o[k];
}

// LT: per-lane thresholds (lane_t); two instantiations, see k_reset in kernels.hip
template <bool LT>
__global__ __launch_bounds__(kBlock) void k_generic_reset(GenericParams P, GenericPool M,
                                                           int64_t n, const uint8_t* mask,
                                                           const uint64_t* eps, double* obs,
                                                           const uint64_t* lane_t) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  if constexpr (LT) P.t_alpha = lane_t[i];  // (the start draws nothing; kept for symmetry)
  GenericLane L = M.lanes[i];
  const GenericBlocks B = lane_blocks(M, P, i);
  if (mask == nullptr || mask[i]) generic::generic_start(B, L, eps ? eps[i] : (uint64_t)i);
  if (L.live == 0) {  // never reset (the pool's headers start zeroed): no DAG to observe
    for (int k = 0; k < 5; ++k) obs[5 * i + k] = 0.0;
    return;
  }
  lane_observe(B, L, obs + 5 * i);
  M.lanes[i] = L;
}

// head_k > 0: the actions are indices of the categorical head of 1 + 2 head_k actions
// (generic_head_action); 0: the reference's integer form
template <bool LT>
__global__ __launch_bounds__(kBlock) void k_generic_step(GenericParams P, uint64_t seed,
                                                          GenericPool M, int64_t n,
                                                          const int32_t* actions, int32_t head_k,
                                                          StepBuffers out,
                                                          const uint64_t* lane_t) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  if constexpr (LT) P.t_alpha = lane_t[i];
  GenericLane L = M.lanes[i];
  const GenericBlocks B = lane_blocks(M, P, i);
  int32_t a = actions[i];
  if (head_k > 0) a = generic::generic_head_action(a, head_k);
  generic::GenericStep t;
  bool done = true;
  if (L.live != 0) {
    done = generic::generic_env_step(P, make_stream(seed, L.ep), B, L, a, &t, [](bool, bool) {});
  } else {
    t = generic::GenericStep{0, 0, 0, 0, 0, false};
  }
  out.reward[i] = (double)t.reward_attacker;
  out.done[i] = done ? 1 : 0;
  out.status[i] = L.status;
  if (out.era) {
    out.era[i] = (double)L.era;
    out.erd[i] = (double)L.erd;
    out.eprog[i] = (double)L.eprog;
    out.ect[i] = 0.0;
    out.est[i] = 0.0;
    out.esteps[i] = L.steps;
    out.eacts[i] = L.mined + 1;
    out.hh[i] = L.live != 0 ? (int32_t)B.height[L.dentry] : 0;
    out.hm[i] = -1;
  }
  if (L.live != 0) {
    lane_observe(B, L, out.obs + 5 * i);
    out.status[i] = L.status;  // (the observation's checks of nakamoto.rs:94-98)
    M.lanes[i] = L;
  } else {
    for (int k = 0; k < 5; ++k) out.obs[5 * i + k] = 0.0;
  }
}

__global__ __launch_bounds__(kBlock) void k_generic_observe_fields(GenericParams P,
                                                                    GenericPool M, int64_t n,
                                                                    int32_t* f) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  GenericLane L = M.lanes[i];
  generic::GenericObs o{0, 0, 0};
  if (L.live != 0) o = generic::generic_observe_fields(lane_blocks(M, P, i), L);
  f[7 * i] = o.a;
  f[7 * i + 1] = o.d;
  f[7 * i + 2] = o.mf;
  f[7 * i + 3] = L.live != 0 ? L.n_rel : 0;
  f[7 * i + 4] = L.live != 0 ? L.n_con : 0;
  f[7 * i + 5] = L.live != 0 ? L.n_blocks : 0;
  f[7 * i + 6] = L.live != 0 ? L.last_rewrite : 0;
}

// LaneCursor: activations are the blocks mined plus one (the StepBuffers' eacts)
__global__ __launch_bounds__(kBlock) void k_generic_cursor(const GenericLane* lanes, int64_t n,
                                                            LaneCursor c) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const bool live = lanes[i].live != 0;
  c.ep[i] = live ? lanes[i].ep : (uint64_t)i;
  c.steps[i] = live ? lanes[i].steps : 0;
  c.acts[i] = live ? lanes[i].mined + 1 : 0;
}

static unsigned grid_of(int64_t n) { return (unsigned)((n + kBlock - 1) / kBlock); }

size_t generic_header_bytes(int64_t n) { return (size_t)n * sizeof(GenericLane); }

size_t generic_pool_bytes(const GenericParams& P, int64_t n) {
  return generic_header_bytes(n) + (size_t)n * generic::generic_region_bytes(P.max_steps);
}

static GenericPool pool_of(const GenericParams& P, void* pool, int64_t n) {
  GenericPool M;
  M.lanes = (GenericLane*)pool;
  M.regions = (uint8_t*)pool + generic_header_bytes(n);
  M.region = generic::generic_region_bytes(P.max_steps);
  return M;
}

hipError_t launch_generic_reset(const GenericParams& P, void* pool, int64_t n,
                                const uint8_t* mask, const uint64_t* eps, double* obs,
                                hipStream_t st, const uint64_t* lane_t) {
  const GenericPool M = pool_of(P, pool, n);
  if (lane_t)
    hipLaunchKernelGGL(k_generic_reset<true>, dim3(grid_of(n)), dim3(kBlock), 0, st, P, M, n,
                       mask, eps, obs, lane_t);
  else
    hipLaunchKernelGGL(k_generic_reset<false>, dim3(grid_of(n)), dim3(kBlock), 0, st, P, M, n,
                       mask, eps, obs, lane_t);
  return hipGetLastError();
}

hipError_t launch_generic_step(const GenericParams& P, uint64_t seed, void* pool, int64_t n,
                               const int32_t* actions, int32_t head_k, const StepBuffers& b,
                               hipStream_t st, const uint64_t* lane_t) {
  const GenericPool M = pool_of(P, pool, n);
  if (lane_t)
    hipLaunchKernelGGL(k_generic_step<true>, dim3(grid_of(n)), dim3(kBlock), 0, st, P, seed, M,
                       n, actions, head_k, b, lane_t);
  else
    hipLaunchKernelGGL(k_generic_step<false>, dim3(grid_of(n)), dim3(kBlock), 0, st, P, seed, M,
                       n, actions, head_k, b, lane_t);
  return hipGetLastError();
}

hipError_t launch_generic_observe_fields(const GenericParams& P, void* pool, int64_t n,
                                         int32_t* f, hipStream_t st) {
  hipLaunchKernelGGL(k_generic_observe_fields, dim3(grid_of(n)), dim3(kBlock), 0, st, P,
                     pool_of(P, pool, n), n, f);
  return hipGetLastError();
}

hipError_t launch_generic_cursor(const void* pool, int64_t n, const LaneCursor& c,
                                 hipStream_t st) {
  hipLaunchKernelGGL(k_generic_cursor, dim3(grid_of(n)), dim3(kBlock), 0, st,
                     (const GenericLane*)pool, n, c);
  return hipGetLastError();
}

}  // namespace cpr
