// Parameter structs and launchers of the Q-learning kernels (kernels_dqn.hip): the
// epsilon-greedy forward that fills a replay slot, the slot's next observation, the training
// forward with the target network and the TD / Huber epilogue, its statistics and the Polyak
// update. The backward, the norm clip and Adam are the learner's (ppo.h).
// DESIGN.md §4.14 "Q-learning".
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include "policy_net.h"
#include "ppo.h"

namespace cpr {

// keyed-stream tags (cpr_stream.h has 0 and 0x1.. - 0x6.., lane_env.h 0x7.., the learner's
// permutations 0x8..)
constexpr uint32_t TAG_EXPLORE = 0x90000000u;  // (episode, step index): the exploration coin
constexpr uint32_t TAG_REPLAY = 0xA0000000u;   // (update, gradient step, row >> 1): sampling

// per-step statistics on the device, f64, in the learner's stats array: row means, and the
// gradient norm where the learner's kernels put it (kPpoGradNorm)
enum { kDqnLoss = 0, kDqnAbsTd = 1, kDqnQ = 2, kDqnTarget = 3 };
constexpr int kDqnRowStats = 4;
static_assert(kDqnRowStats <= kPpoGradNorm, "the row statistics stand below the gradient norm");

// one slot of the ring, or n rows of it: transitions as structure of arrays
struct DqnRows {
  float* obs;       // [n][obs_len] the f32 policy input's observation columns
  float* next_obs;  // [n][obs_len]
  double* alpha;    // [n] the row's lane alpha
  int32_t* action;  // [n]
  double* reward;   // [n]
  uint8_t* done;    // [n]
};

// the acting forward over the n lanes: the pi trunk alone, the epsilon-greedy action, and the
// slot's obs / alpha / action
struct DqnAct {
  const double* obs;         // [n][obs_len]
  int64_t n;
  double epsilon;
  uint64_t seed;
  const uint64_t* ep;        // [n] lane cursors
  const int64_t* step;       // [n]
  const double* lane_alpha;  // [n] or null: cfg_alpha
  int32_t alpha_col;         // the input's alpha column, -1: constants only
  double cfg_alpha;
  int32_t* action;           // [n] for the step kernels
  DqnRows slot;              // obs, alpha, action are written
};
hipError_t launch_dqn_act(const PolNet& N, const DqnAct& A, hipStream_t st);

// next_obs of a slot from the reset kernel's f64 observations: cells = n * obs_len
hipError_t launch_dqn_store(const double* obs, int64_t cells, float* next_obs, hipStream_t st);

// the training forward over rows idx[0 .. B) of N transitions: the online network on obs with
// the saved activations of k_ppo_forward, the target network on next_obs, the TD target and
// the Huber loss. Inputs are the ring's f32 rows (obs32 / next32) or the caller's f64 rows.
struct DqnFwd {
  const float* obs32;
  const float* next32;
  const double* obs64;
  const double* next64;
  const double* alpha;  // [N] or null
  int32_t alpha_col;
  const int32_t* action;
  const double* reward;
  const uint8_t* done;
  const int64_t* idx;  // [B]
  int64_t B, N;
  double gamma;
  float* xin;                 // [B][kPolInStride]
  float* act[kPolMaxDepth];   // [layer] [B][width_pi]
  float* dlogits;             // [B][n_actions]
  double* partial;            // [workgroups][kDqnRowStats]
};
hipError_t launch_dqn_forward(const PolNet& online, const PolNet& target, const DqnFwd& F,
                              hipStream_t st);
// stats[0 .. kDqnRowStats) = the partials summed in workgroup order / B; acc (optional) += them
hipError_t launch_dqn_stats(const double* partial, int64_t blocks, int64_t B, double* stats,
                            double* acc, hipStream_t st);

// t[i] = (t[i] omt) + (p[i] tf), i < n; omt = 0: t[i] = p[i]
hipError_t launch_polyak(float* t, const float* p, int64_t n, float omt, float tf, hipStream_t st);

int64_t dqn_lds_limit();

}  // namespace cpr
