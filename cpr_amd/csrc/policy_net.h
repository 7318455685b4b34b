// Parameter structs and launchers of the neural-network policy kernels
// (kernels_policy.hip): a batched actor-critic MLP evaluated next to the lockstep lanes
// (cpr_policy_net_forward, cpr_rollout_net). DESIGN.md §4.14.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include "../../include/cpr_hip.h"

namespace cpr {

constexpr int kPolMaxDepth = 4;     // hidden layers per trunk
constexpr int kPolMaxWidth = 512;   // units of a hidden layer (a multiple of 16)
constexpr int kPolMaxExtra = 8;     // constants appended to the observation
constexpr int kPolMaxActions = 24;  // widest action head (Ethereum)
constexpr int kPolRows = 64;        // rows (lanes) a workgroup owns
constexpr int kPolKT = 32;          // K extent of one staged weight chunk
constexpr int kPolNT = 64;          // output units of one staged weight chunk (16 per wave)
constexpr int kPolInStride = 20;    // floats per row of the input tile (obs_len + n_extra <= 18)
constexpr int kPolWsStride = kPolKT + 4;
constexpr int kPolLogitStride = kPolMaxActions + 1;

// one Linear layer: W [n_out][n_in] row-major (torch.nn.Linear), b [n_out]; device pointers
struct PolLayer {
  const float* W;
  const float* b;
  int32_t n_in, n_out;
};

// the network on the device: layers 0 .. depth-1 of a trunk are its hidden layers, layer
// `depth` its head (n_actions / 1 outputs)
struct PolNet {
  int32_t obs_len, n_extra, depth, n_actions;
  int32_t width_pi, width_vf;
  float extra[kPolMaxExtra];
  PolLayer pi[kPolMaxDepth + 1];
  PolLayer vf[kPolMaxDepth + 1];
};

// one forward over n rows (device pointers; outputs optional)
struct PolIO {
  const double* obs;    // [n][obs_len]
  int64_t n;
  int32_t deterministic;
  uint64_t seed;
  const uint64_t* ep;   // [n] episode of each row's draw; null: episode0 + row
  uint64_t episode0;
  const int64_t* step;  // [n] episode step index of each row's draw; null: 0
  int32_t* action;      // [n]
  double* logp;         // [n]
  double* value;        // [n]
  float* logits;        // [n][n_actions]
  // lane env (cpr_lane_env_set): extra column alpha_col of row r is (float)lane_alpha[r]
  // instead of the constant; null / -1: constants only
  const double* lane_alpha;  // [n]
  int32_t alpha_col;
};

// floats per row of a hidden-activation tile: the padding makes the 16 rows x 4 k of an
// MFMA operand read fall on 64 distinct LDS banks (width is a multiple of 16)
inline int64_t policy_act_stride(int32_t width) { return (int64_t)width + 4; }

// dynamic LDS bytes of k_policy_forward (the budget formula of DESIGN.md §4.14): the input
// tile, one hidden tile (two from depth 2 on: a layer reads one and writes the other) of the
// wider trunk, the weight chunk, logits and values of the workgroup's rows
inline int64_t policy_lds_bytes(int32_t depth, int32_t width_pi, int32_t width_vf) {
  const int32_t w = width_pi > width_vf ? width_pi : width_vf;
  const int64_t hidden = (int64_t)kPolRows * policy_act_stride(w) * (depth >= 2 ? 2 : 1);
  const int64_t fixed = (int64_t)kPolRows * kPolInStride + (int64_t)kPolNT * kPolWsStride +
                        (int64_t)kPolRows * kPolLogitStride + kPolRows;
  return 4 * (hidden + fixed);
}

// the most dynamic LDS k_policy_forward may ask for on the current device
int64_t policy_lds_limit();
hipError_t launch_policy_forward(const PolNet& N, const PolIO& io, hipStream_t st);

// per-step bookkeeping of cpr_rollout_net over n lanes (device pointers)
struct PolCollect {
  // the step's outputs (StepBuffers of the lockstep step kernels)
  const double* reward;
  const uint8_t* done;
  const double* era;
  const double* erd;
  const double* eprog;
  const int64_t* esteps;
  const int64_t* eacts;
  const int32_t* hh;
  const uint32_t* status;
  int32_t orphans_from_progress;  // B_k, Tailstorm: orphans = activations - progress
  // step-major outputs at this step (optional)
  double* out_reward;
  uint8_t* out_done;
  // lane cursors: episode id, episode step index, activations of the episode already counted
  uint64_t* ep;
  int64_t* step;
  int64_t* acts0;
  uint8_t* mask;  // reset mask of this step
  cpr_summary* sum;
  // lane env (lane_env.h): reward wrapper and shape of out_reward, the lanes' alphas and
  // dense accumulators (null: the engine's reward), the unwrapped reward (optional)
  int32_t gym_reward, reward_shape;
  double dense_target;
  const double* lane_alpha;
  double* dense_acc;
  double* out_engine_reward;
};
hipError_t launch_policy_collect(const PolCollect& C, int64_t n, hipStream_t st);
// The assumption schedule (lane_env.h): lanes with mask[i] != 0 (null: all) take the
// threshold and alpha of their new episode eps[i] (null: the lane index) from the batch's
// table and zero their dense accumulator; out_alpha (optional) gets every lane's alpha.
// Runs before every lockstep reset launch of a batch with a lane env.
struct LaneAssign {
  const uint8_t* mask;
  const uint64_t* eps;
  uint64_t seed;
  int32_t n_alpha;
  int32_t schedule;       // enum cpr_alpha_schedule (lane_env.h lane_alpha_entry)
  const uint64_t* tab_t;  // [n_alpha] alpha_threshold of each entry
  const double* tab_a;    // [n_alpha]
  uint64_t* lane_t;       // [n]
  double* lane_alpha;     // [n]
  double* dense_acc;      // [n]
  double* out_alpha;      // [n]
};
hipError_t launch_lane_assign(const LaneAssign& A, int64_t n, hipStream_t st);

// per-step bookkeeping of cpr_eval_net over n lanes (device pointers): the wrapped and shaped
// reward as in PolCollect, summed per lane in step order; at a done of an episode of the set
// [first, first + n_set) one cpr_eval_record at slot episode - first
struct EvalCollect {
  const double* reward;
  const uint8_t* done;
  const double* era;
  const double* erd;
  const double* eprog;
  const double* ect;
  const double* est;
  const int64_t* esteps;
  const int64_t* eacts;
  const int32_t* hh;
  const uint32_t* status;
  int32_t orphans_from_progress;
  uint64_t* ep;    // lane cursors: episode id, episode step index
  int64_t* step;
  uint8_t* mask;   // reset mask of this step
  double* ep_reward;  // [n] erw_episode_reward of the lane's episode so far
  // lane env (null lane_alpha: the engine's reward, every episode at cfg_alpha, entry 0)
  int32_t gym_reward, reward_shape;
  double dense_target;
  const double* lane_alpha;
  double* dense_acc;
  double cfg_alpha;
  int32_t n_alpha, schedule;
  uint64_t seed;
  // the set and its outputs
  uint64_t first;
  int64_t n_set;
  cpr_eval_record* records;       // [n_set]
  unsigned long long* finished;   // episodes of the set that have finished
};
hipError_t launch_eval_collect(const EvalCollect& C, int64_t n, hipStream_t st);

// After the loop, one workgroup per alpha j < n_alpha over the records at slots s with
// (first + s) mod n_alpha = j: that alpha's cpr_summary (sums, zeroed by the caller) and
// cpr_eval_alpha (eval.h has the order).
struct EvalReduce {
  const cpr_eval_record* records;
  uint64_t first;
  int64_t per_alpha;      // records of each alpha
  int32_t n_alpha;
  const double* tab_a;    // [n_alpha] the table; null: cfg_alpha
  double cfg_alpha;
  cpr_summary* sums;      // [n_alpha]
  cpr_eval_alpha* out;    // [n_alpha]
};
hipError_t launch_eval_reduce(const EvalReduce& R, hipStream_t st);

// after the last step: activations of the episodes still running (acts[i] - acts0[i])
hipError_t launch_policy_tail(const int64_t* acts, const int64_t* acts0, int64_t n,
                              cpr_summary* sum, hipStream_t st);

}  // namespace cpr
