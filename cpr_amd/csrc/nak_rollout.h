// The closed-form lockstep lane of cpr_reset / cpr_step / cpr_rollout (Nakamoto) and one
// rollout step of it: batch policy on the lane's own observation fields, action log, step
// (apply, resolve, activate), the done rule of engine.ml:225-231, reward (engine.ml:223) and
// the VecEnv auto-reset bookkeeping (episode id + n_lanes). Compiles for the host like
// nakamoto_lane.h (tests/native_rollout runs it beside the oracle's gym); the device loop
// around it is k_nak_rollout (kernels.hip).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "nakamoto_lane.h"

#pragma clang fp contract(off)

namespace cpr {

// lane status bits whose episodes the closed form cannot vouch for
constexpr uint32_t kInexact = ST_OVERLAP | ST_DEEP_FORK | ST_TIE_UNRESOLVED | ST_STALE_TIME;

struct LockLane {
  NakLane L;
  uint64_t ep;
  int64_t steps;
  double last_ra;
  // 0 = never reset, 1 = running; 2 = (between the passes of one cpr_rollout call only) the
  // lane claimed its exact-engine slot at the step it has just taken on the closed form, and
  // the exact pass has yet to replay the episode there and finish that step
  int32_t live;
  int32_t exact;  // 1 + the exact-engine slot this lane runs on, 0 = the closed form
};

__host__ __device__ inline CPR_AI Stream roll_stream(uint64_t seed, uint64_t ep) {
  Stream S;
  S.k0 = (uint32_t)seed;
  S.k1 = (uint32_t)(seed >> 32);
  S.e0 = (uint32_t)ep;
  S.e1 = (uint32_t)(ep >> 32);
  return S;
}

// engine.ml:122-170 on the closed form: episode `ep` up to the attacker's first interaction
__host__ __device__ inline CPR_AI void roll_reset(LockLane& LL, const NakParams& P,
                                                  uint64_t seed, const LaneMem& M, uint64_t ep) {
  LL.L.init();
  LL.L.activate(P, roll_stream(seed, ep), M);
  LL.ep = ep;
  LL.steps = 0;
  LL.last_ra = 0.0;
  LL.live = 1;
}

struct RollStep {
  int32_t action;
  int32_t done;
  double ra;      // attacker reward of the head after the step
  double reward;  // ra - the lane's last_ra (engine.ml:223)
  BRef head;
};

// One step with the batch policy, as cpr_policy_actions + k_step: the action is logged at
// alog[steps] while the log has room (alog = null: no log). LL.last_ra is left alone: the
// caller either keeps the step (roll_keep) or hands the lane to the exact engine, which
// replays the episode from the log and needs the reward baseline of before this step.
__host__ __device__ inline CPR_AI RollStep roll_step(LockLane& LL, const NakParams& P,
                                                     uint64_t seed, const LaneMem& M,
                                                     uint8_t* alog, int64_t alog_cap) {
  RollStep r;
  int32_t h, a, d, ev;
  LL.L.observe(&h, &a, &d, &ev);
  r.action = nak_policy(P.policy, h, a, ev, P.table, P.table_dim);
  if (alog != nullptr && LL.steps < alog_cap) alog[LL.steps] = (uint8_t)r.action;
  const Stream S = roll_stream(seed, LL.ep);
  LL.L.apply(r.action);
  LL.L.resolve(P, S, M);
  LL.L.activate(P, S, M);
  LL.steps += 1;
  r.head = LL.L.head(P, M);
  const double progress = (double)r.head.h;
  r.done = !(LL.steps < P.max_steps && progress < P.max_progress && LL.L.t < P.max_time) ? 1 : 0;
  r.ra = (double)r.head.ra;
  r.reward = r.ra - LL.last_ra;
  return r;
}

// the step stands: the reward baseline moves on, and a finished episode's lane restarts at
// episode id + n_lanes (the caller has read what it needs of the finished episode)
__host__ __device__ inline CPR_AI void roll_keep(LockLane& LL, const NakParams& P, uint64_t seed,
                                                 const LaneMem& M, const RollStep& r,
                                                 int64_t n_lanes) {
  LL.last_ra = r.ra;
  if (r.done) roll_reset(LL, P, seed, M, LL.ep + (uint64_t)n_lanes);
}

}  // namespace cpr
