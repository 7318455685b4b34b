// The gym layers of cpr-v0 over the lockstep lanes (cpr_lane_env_set): which
// alpha an episode runs at, and the reward wrappers of gym/ocaml/cpr_gym/wrappers.py and
// experiments/train/ppo.py:221-232 on a step's outputs. Host-compilable, so that a native
// test pins both rules (tests/native_laneenv); kernels_policy.hip runs the same functions.
#pragma once
#include <stdint.h>

#include "../../include/cpr_hip.h"
#include "cpr_stream.h"

#pragma clang fp contract(off)

namespace cpr {

// the assumption schedule's draw: u53(w0, w1) of block (0, TAG_ASSUME) of the episode's stream
constexpr uint32_t TAG_ASSUME = 0x70000000u;
constexpr int32_t kLaneEnvMaxAlpha = 4096;

// random.choice over a table of n_alpha entries (ppo.py:117-118), keyed by (seed, episode)
// alone: entry min(n_alpha - 1, (int)(u n_alpha))
__host__ __device__ inline int32_t lane_alpha_index(uint64_t seed, uint64_t episode,
                                                    int32_t n_alpha) {
  const Words4 w = philox4x32_10((uint32_t)episode, (uint32_t)(episode >> 32), 0u, TAG_ASSUME,
                                 (uint32_t)seed, (uint32_t)(seed >> 32));
  const int32_t i = (int32_t)(u53(w.w0, w.w1) * (double)n_alpha);
  return i < n_alpha - 1 ? i : n_alpha - 1;
}

// the table entry of episode `episode` under a schedule (enum cpr_alpha_schedule):
// CPR_SCHEDULE_CYCLE is itertools.cycle over the table (wrappers.py:186-193) as a function of
// the episode id alone, entry episode mod n_alpha; anything else the keyed choice above
__host__ __device__ inline int32_t lane_alpha_entry(int32_t schedule, uint64_t seed,
                                                    uint64_t episode, int32_t n_alpha) {
  if (schedule == CPR_SCHEDULE_CYCLE) return (int32_t)(episode % (uint64_t)n_alpha);
  return lane_alpha_index(seed, episode, n_alpha);
}

// what the wrappers read of one engine step (engine.ml:223-241)
struct GymStepInfo {
  double reward;    // engine.ml:223
  bool done;
  double era, erd;  // episode_reward_attacker / _defender
  double progress;  // episode_progress
  int64_t n_activations;
};

// wrappers.py:8-113 on one step, f64, one rounding per operation. *acc is the dense wrapper's
// drpb_acc (zeroed at the lane's reset); `target` its episode_len. A dense episode that ends
// with progress 0 gets no correction (the reference divides by zero there and raises).
__host__ __device__ inline double gym_reward(int32_t scheme, double target, const GymStepInfo& s,
                                             double* acc) {
  switch (scheme) {
    case CPR_GYM_REWARD_SPARSE_RELATIVE: {
      if (!s.done) return 0.0;
      const double total = s.era + s.erd;
      return total != 0.0 ? s.era / total : 0.0;
    }
    case CPR_GYM_REWARD_SPARSE_PER_PROGRESS:
      if (!s.done) return 0.0;
      return s.progress != 0.0 ? s.era / s.progress : 0.0;
    case CPR_GYM_REWARD_DENSE_PER_PROGRESS: {
      const double factor = 1.0 / target;
      double r = s.reward * factor;
      *acc = *acc + r;
      if (s.done && s.progress != target && s.progress != 0.0) {
        const double miss = target - s.progress;
        r = r + miss * *acc / s.progress;
      }
      return r;
    }
    default:
      return s.reward;
  }
}

// envs.py:149-150 (r / alpha) and ppo.py:223-230 (cut) on the wrapped reward
__host__ __device__ inline double shape_reward(int32_t shape, double r, double alpha,
                                               const GymStepInfo& s) {
  if (shape == CPR_SHAPE_PER_ALPHA) return r / alpha;
  if (shape == CPR_SHAPE_CUT) {
    if (r <= 0.0 || s.progress <= 0.0) return 0.0;
    const double orphans = (double)s.n_activations / s.progress;
    if (orphans <= 1.05) return r * 0.9 / alpha;
    return r / alpha;
  }
  return r;
}

}  // namespace cpr
