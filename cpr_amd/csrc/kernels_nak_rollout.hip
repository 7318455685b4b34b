// Device rollout of the Nakamoto lockstep lanes for gfx950 (cpr_rollout): the closed-form
// pass and the exact pass. A translation unit of its own: kernels.hip pins the stream's seed
// words to scalar registers for its fused kernels (CPR_UNIFORM_SEED), which this loop, with
// its per-lane trip count, does not compile under.
#include <hip/hip_runtime.h>

#include "../../include/cpr_hip.h"
#include "kernels.h"
#include "kernels_lock.h"
#include "nak_rollout.h"
#include "nakamoto_lane.h"
#include "summary.h"

#pragma clang fp contract(off)

namespace cpr {

// ---- device rollout of the lockstep lanes (cpr_rollout)
//
// Two passes per round, one thread per lane each, sharing a per-lane step cursor. The
// closed-form pass keeps the lane's LockLane in registers and steps it (nak_rollout.h) to
// the end of the rollout, or to the step whose flags (kInexact) make it claim an
// exact-engine slot; that step's outputs are not written. The exact pass replays such a
// lane's episode from its action log (as k_lock_exact), which finishes that step, and steps
// it on with the batch policy until its episode ends (summary, slot back to the free stack,
// restart on the closed form) or the rollout does. Slots are only popped in the closed-form
// pass and only pushed in the exact pass, so the free stack never sees both in one kernel.

__global__ __launch_bounds__(kBlock) void k_nak_rollout(NakParams P, uint64_t seed,
                                                         LockBuffers B, int64_t n,
                                                         RollBuffers R, int unit,
                                                         const double* tab_nn,
                                                         const double* tab_sg, int32_t tab_n) {
  __shared__ int32_t hist[CPR_HIST_BINS];
  __shared__ unsigned long long acc_w[13];
  LdsAcc acc{acc_w};
  acc.init();
  if (threadIdx.x < CPR_HIST_BINS) hist[threadIdx.x] = 0;
  __syncthreads();
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) {
    LockLane* const slot = (LockLane*)B.lanes + i;
    int64_t t = R.cursor[i];
    if (slot->exact == 0 && t < R.n_steps) {
      LockLane LL = *slot;
      const LaneMem M = lock_mem(P, B, i, n);
      uint8_t* const alog = B.alog ? B.alog + i * B.alog_cap : nullptr;
      // steps and activations of this call that no finished episode has added to the summary
      int64_t dsteps = 0, dacts = 0;
      if (!LL.live) {
        roll_reset(LL, P, seed, M, (uint64_t)i);
        dacts += LL.L.k;
      }
      for (; t < R.n_steps; ++t) {
        const int32_t k0 = LL.L.k;
        const RollStep r = roll_step(LL, P, seed, M, alog, B.alog_cap);
        dacts += LL.L.k - k0;
        if (alog != nullptr && (LL.L.status & kInexact) != 0u && LL.steps <= B.alog_cap) {
          // the lane leaves the closed form (k_lock_exact's rule, retried at every later
          // step while every slot is taken: the lane keeps its flags until then)
          const int32_t top = atomicSub(B.efree + B.n_slots, 1) - 1;
          if (top >= 0) {
            LL.exact = B.efree[top] + 1;
            LL.live = 2;
            break;
          }
          atomicAdd(B.efree + B.n_slots, 1);
        }
        ++dsteps;
        const int64_t c = t * n + i;
        if (R.reward) R.reward[c] = r.reward;
        if (R.done) R.done[c] = (uint8_t)r.done;
        if (r.done) {
          const BRef& hd = r.head;
          const double rel = hd.h != 0 ? (double)hd.ra / (double)hd.h : 0.0;
          acc.episode((int64_t)hd.ra << 20, (int64_t)(hd.h - hd.ra) << 20, (int64_t)hd.h << 20,
                      rel, hd.h, LL.steps, LL.L.k, LL.L.status, hist);
          dsteps -= LL.steps;
          dacts -= LL.L.k;
        }
        roll_keep(LL, P, seed, M, r, n);
        if (r.done) dacts += LL.L.k;  // the new episode's first activation
        if (R.obs) write_obs(LL.L, unit, tab_nn, tab_sg, tab_n, R.obs + 4 * c);
      }
      *slot = LL;
      R.cursor[i] = t;
      if (dsteps) atomicAdd(&acc_w[1], (unsigned long long)dsteps);
      if (dacts) atomicAdd(&acc_w[2], (unsigned long long)dacts);
    }
  }
  __syncthreads();
  acc.flush(hist, R.sum);
}

__global__ __launch_bounds__(kBlock) void k_nak_rollout_exact(NakParams P, eth::EthParams EP,
                                                               uint64_t seed, LockBuffers B,
                                                               int64_t n, RollBuffers R, int unit,
                                                               const double* tab_nn,
                                                               const double* tab_sg,
                                                               int32_t tab_n) {
  __shared__ int32_t hist[CPR_HIST_BINS];
  if (threadIdx.x < CPR_HIST_BINS) hist[threadIdx.x] = 0;
  __syncthreads();
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  Acc acc = {};
  int64_t steps_all = 0, acts_all = 0;
  if (i < n) {
    LockLane& LL = ((LockLane*)B.lanes)[i];
    int64_t t = R.cursor[i];
    if (LL.exact > 0 && t < R.n_steps) {
      eth::EthLane* slots = (eth::EthLane*)B.eslots;
      const int32_t slot = LL.exact - 1;
      const eth::EthMem M = lock_exact_mem(EP, B, slot);
      const Stream S = make_stream(seed, LL.ep);
      uint8_t* const alog = B.alog + i * B.alog_cap;
      eth::EthLane E;
      if (LL.live != 2) E = slots[slot];
      bool over = false;  // the lane's episode ended: it is back on the closed form
      for (; t < R.n_steps && !over; ++t) {
        int32_t hd = 0;
        bool done = false;
        if (LL.live == 2) {
          // the closed-form pass took this step and claimed the slot: the episode again
          // from its first draw with the logged actions (k_lock_exact's first branch)
          E.gym_reset(EP, S, M);
          for (int64_t s = 0; s < LL.steps; ++s)
            hd = E.gym_step(EP, S, M, nak_to_eth_action(alog[s]), &done);
          LL.live = 1;
          acts_all += E.c_act - LL.L.k;  // the closed-form pass counted its own
        } else {
          const eth::EthObs o = E.observe(EP, M, false);
          const int32_t a = nak_policy(P.policy, o.public_height, o.private_height, o.event,
                                       P.table, P.table_dim);
          if (LL.steps < B.alog_cap) alog[LL.steps] = (uint8_t)a;
          const int32_t c0 = E.c_act;
          hd = E.gym_step(EP, S, M, nak_to_eth_action(a), &done);
          LL.steps += 1;
          acts_all += E.c_act - c0;
        }
        ++steps_all;
        const eth::EBlock h = E.B(EP, M, hd);
        const double ra = (double)(h.rew_att / 32);  // 1 per block in Nakamoto mode
        const int64_t c = t * n + i;
        if (R.reward) R.reward[c] = ra - LL.last_ra;  // engine.ml:223
        if (R.done) R.done[c] = done ? 1 : 0;
        LL.last_ra = ra;
        if (done) {
          const int32_t a = h.rew_att, d = h.rew_def;  // units of 1/32
          const double rel = (a + d) != 0 ? (double)a / (double)(a + d) : 0.0;
          acc_episode(acc, (int64_t)a << 15, (int64_t)d << 15, (int64_t)h.work << 20, rel,
                      h.height, E.steps, E.c_act, LL.L.status | E.status | CPR_ST_EXACT_RERUN,
                      hist);
          const int32_t top = atomicAdd(B.efree + B.n_slots, 1);
          B.efree[top] = slot;
          LockLane N;
          roll_reset(N, P, seed, lock_mem(P, B, i, n), LL.ep + (uint64_t)n);
          N.exact = 0;
          LL = N;
          acts_all += N.L.k;
          over = true;
          if (R.obs) write_obs(N.L, unit, tab_nn, tab_sg, tab_n, R.obs + 4 * c);
        } else if (R.obs) {
          const eth::EthObs o = E.observe(EP, M, false);
          write_obs_fields(o.public_height, o.private_height, o.diff_height, o.event, unit,
                           tab_nn, tab_sg, tab_n, R.obs + 4 * c);
        }
      }
      if (!over) slots[slot] = E;
      R.cursor[i] = t;
    }
    // back on the closed form with steps to take: the host runs another round
    if (t < R.n_steps) atomicAdd(R.left, 1ull);
  }
  acc.steps = steps_all;
  acc.activations = acts_all;
  __syncthreads();
  block_flush(acc, hist, R.sum);
}

// ---------------------------------------------------------------- launchers

hipError_t launch_nak_rollout(const NakParams& P, uint64_t seed, const LockBuffers& B, int64_t n,
                              const RollBuffers& R, int unit, const double* tab_nn,
                              const double* tab_sg, int32_t tab_n, hipStream_t st) {
  const unsigned blocks = (unsigned)((n + kBlock - 1) / kBlock);
  hipLaunchKernelGGL(k_nak_rollout, dim3(blocks), dim3(kBlock), 0, st, P, seed, B, n, R, unit,
                     tab_nn, tab_sg, tab_n);
  return hipGetLastError();
}

hipError_t launch_nak_rollout_exact(const NakParams& P, const eth::EthParams& EP, uint64_t seed,
                                    const LockBuffers& B, int64_t n, const RollBuffers& R,
                                    int unit, const double* tab_nn, const double* tab_sg,
                                    int32_t tab_n, hipStream_t st) {
  if (!B.alog) return hipSuccess;  // no exact engine for this batch: no lane ever moves
  CPR_LAYOUT_GUARD(B.elane_bytes, eth::eth_lane_bytes(EP.cap_b, EP.cap_e, EP.n));
  const unsigned blocks = (unsigned)((n + kBlock - 1) / kBlock);
  hipLaunchKernelGGL(k_nak_rollout_exact, dim3(blocks), dim3(kBlock), 0, st, P, EP, seed, B, n,
                     R, unit, tab_nn, tab_sg, tab_n);
  return hipGetLastError();
}

int nak_rollout_blocks_per_cu() {
  int blocks = 0;
  hipError_t e = hipOccupancyMaxActiveBlocksPerMultiprocessor(&blocks, (const void*)k_nak_rollout,
                                                              kBlock, 0);
  if (e != hipSuccess || blocks <= 0) blocks = 2;
  return blocks;
}

}  // namespace cpr
