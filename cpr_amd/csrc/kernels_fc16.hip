// FC'16 abstract-model kernels for gfx950 (fc16_lane.h):
//   k_fc16_episodes      one lane = one probabilistically terminating episode of
//                        gym/rust/src/fc16.rs, grid-stride over episodes, policy (honest, SM1
//                        or an (a, h, fork) table from cpr_amd.mdp) evaluated in the lane.
//                        Integer state and 32-bit threshold draws only; outcomes reduced like
//                        every episode kernel (summary.h)
//   k_fc16_reset / _step the same lane as a lockstep env (CPR_PROTO_FC16_ENV): one thread per
//                        lane over a small slot, actions by index, lane-env thresholds
//   k_fc16_observe_fields, k_fc16_cursor   (a, h, fork) and the LaneCursor of the slots
//   k_fc16_rollout_net   cpr_rollout_net of those lanes in one launch: the policy network on
//                        the f32 MFMA (policy_layer.h) and the env step in the same workgroup
#include <hip/hip_runtime.h>

#include <algorithm>

#include "../../include/cpr_hip.h"
#include "fc16_lane.h"
#include "kernels.h"
#include "lane_env.h"
#include "policy_layer.h"
#include "policy_net.h"
#include "summary.h"

#pragma clang fp contract(off)

namespace cpr {

__global__ __launch_bounds__(kBlock) void k_fc16_episodes(fc16::Fc16Params P, SeedSource src,
                                                          int64_t n_eps,
                                                          cpr_episode_record* recs,
                                                          cpr_summary* sum) {
  __shared__ int32_t hist[CPR_HIST_BINS];
  if (threadIdx.x < CPR_HIST_BINS) hist[threadIdx.x] = 0;
  __syncthreads();
  const int64_t tid = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int64_t nthreads = (int64_t)gridDim.x * blockDim.x;
  Acc acc = {};
  for (int64_t e = tid; e < n_eps; e += nthreads) {
    const fc16::Fc16Out o = fc16::fc16_episode(P, src.at(e));
    const int64_t ra = o.reward, rd = o.progress - o.reward;
    const double rel = o.progress != 0 ? (double)ra / (double)o.progress : 0.0;
    // activations: the start block plus one per step (every step mines one block)
    acc_episode(acc, ra << 20, rd << 20, o.progress << 20, rel, o.progress, o.steps,
                o.steps + 1, o.status, hist);
    if (recs) {
      cpr_episode_record r;
      r.reward_attacker = (double)ra;
      r.reward_defender = (double)rd;
      r.progress = (double)o.progress;
      r.chain_time = 0.0;
      r.sim_time = 0.0;
      r.n_steps = o.steps;
      r.n_activations = o.steps + 1;
      r.head_height = (int32_t)o.progress;
      r.head_miner = -1;
      r.status = o.status;
      r.head_work = 0;
      recs[e] = r;
    }
  }
  __syncthreads();
  block_flush(acc, hist, sum);
}

// ---------------------------------------------------------------- the lane as a lockstep env
// (CPR_PROTO_FC16_ENV): one thread per lane over a small slot

struct Fc16Slot {
  uint64_t ep;
  int64_t reward, progress, steps;
  int32_t a, h, fork;
  uint32_t status;
  int32_t live, _pad;
};

__device__ inline fc16::Fc16State slot_state(const Fc16Slot& SL) {
  return fc16::Fc16State{SL.a, SL.h, SL.fork, SL.steps};
}

__device__ inline void slot_reset(const fc16::Fc16Params& P, uint64_t seed, Fc16Slot& SL,
                                  uint64_t ep) {
  const fc16::Fc16State s = fc16::fc16_start(P, make_stream(seed, ep));
  SL.ep = ep;
  SL.reward = 0;
  SL.progress = 0;
  SL.steps = 0;
  SL.a = s.a;
  SL.h = s.h;
  SL.fork = s.fork;
  SL.status = 0u;
  SL.live = 1;
  SL._pad = 0;
}

// What one env step leaves in the slot and pays: the engine reward and whether the episode is
// over (terminated, or max_steps steps without termination: CPR_ST_CAPACITY, as the fused
// lane's truncation). Shared by k_fc16_step and k_fc16_rollout_net.
__device__ inline bool slot_step(const fc16::Fc16Params& P, uint64_t seed, Fc16Slot& SL,
                                 int32_t index, double* reward) {
  fc16::Fc16State s = slot_state(SL);
  const fc16::Fc16Step t =
      fc16::fc16_step(P, make_stream(seed, SL.ep), s, fc16::fc16_action_name(s.a, s.h, index));
  SL.a = s.a;
  SL.h = s.h;
  SL.fork = s.fork;
  SL.steps = s.steps;
  SL.reward += t.reward;
  SL.progress += t.progress;
  bool done = t.terminated;
  if (!done && SL.steps >= P.max_steps) {
    SL.status |= (uint32_t)CPR_ST_CAPACITY;
    done = true;
  }
  *reward = (double)t.reward;
  return done;
}

// LT: per-lane thresholds (lane_t); two instantiations, see k_reset in kernels.hip
template <bool LT>
__global__ __launch_bounds__(kBlock) void k_fc16_reset(fc16::Fc16Params P, uint64_t seed,
                                                        Fc16Slot* slots, int64_t n,
                                                        const uint8_t* mask, const uint64_t* eps,
                                                        double* obs, const uint64_t* lane_t) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  if constexpr (LT) P.t_alpha = lane_t[i];  // the lane's own alpha (cpr_lane_env_set)
  Fc16Slot SL = slots[i];
  if (mask == nullptr || mask[i]) {
    slot_reset(P, seed, SL, eps ? eps[i] : (uint64_t)i);
    slots[i] = SL;
  }
  fc16::fc16_observe(slot_state(SL), obs + 3 * i);
}

template <bool LT>
__global__ __launch_bounds__(kBlock) void k_fc16_step(fc16::Fc16Params P, uint64_t seed,
                                                       Fc16Slot* slots, int64_t n,
                                                       const int32_t* actions, StepBuffers out,
                                                       const uint64_t* lane_t) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  if constexpr (LT) P.t_alpha = lane_t[i];
  Fc16Slot SL = slots[i];
  double r;
  const bool done = slot_step(P, seed, SL, actions[i], &r);
  out.reward[i] = r;
  out.done[i] = done ? 1 : 0;
  out.status[i] = SL.status;
  if (out.era) {  // the fused record's mapping (k_fc16_episodes)
    out.era[i] = (double)SL.reward;
    out.erd[i] = (double)(SL.progress - SL.reward);
    out.eprog[i] = (double)SL.progress;
    out.ect[i] = 0.0;
    out.est[i] = 0.0;
    out.esteps[i] = SL.steps;
    out.eacts[i] = SL.steps + 1;
    out.hh[i] = (int32_t)SL.progress;
    out.hm[i] = -1;
  }
  fc16::fc16_observe(slot_state(SL), out.obs + 3 * i);
  slots[i] = SL;
}

__global__ __launch_bounds__(kBlock) void k_fc16_observe_fields(const Fc16Slot* slots, int64_t n,
                                                                 int32_t* f) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  f[3 * i] = slots[i].a;
  f[3 * i + 1] = slots[i].h;
  f[3 * i + 2] = slots[i].fork;
}

// LaneCursor: the start block plus one activation per step
__global__ __launch_bounds__(kBlock) void k_fc16_cursor(const Fc16Slot* slots, int64_t n,
                                                         LaneCursor c) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const bool live = slots[i].live != 0;
  c.ep[i] = live ? slots[i].ep : (uint64_t)i;
  c.steps[i] = live ? slots[i].steps : 0;
  c.acts[i] = live ? slots[i].steps + 1 : 0;
}

// ---------------------------------------------------------------- the one-kernel network rollout
// cpr_rollout_net(_env) of an FC16 env batch without a launch per step: a
// kPolThreads workgroup owns kPolRows lanes for all n_steps steps. Threads 0 .. kPolRows - 1
// hold one lane's slot in registers; per step they write the f32 input tile from it, the whole
// workgroup runs both trunks and heads through pol_layer, and the same threads then do what
// the launch sequence does: the forward's epilogue (pol_choose), the env step (slot_step), the
// collect's reward wrappers, outputs and summary (k_policy_collect), the lane env's assignment
// (k_lane_assign) and the reset (k_fc16_reset) of a finished lane. One more forward gives the
// bootstrap value row.
//
// The rule that keeps the workgroup from hanging: no return and no branch around a barrier.
// Every thread makes the same pol_layer calls; their number depends on kernel arguments alone
// (n_steps, depth), never on a lane's state or on row < n. Rows beyond n are computed on zeros
// and never stored.
__device__ inline void roll_forward(const PolNet& N, int32_t hstride, float* xin, float* ws,
                                    float* lg, float* val, float* h0, float* h1) {
  for (int trunk = 0; trunk < 2; ++trunk) {
    const PolLayer* Ls = trunk == 0 ? N.pi : N.vf;
    const float* src = xin;
    int sstride = kPolInStride;
    for (int l = 0; l < N.depth; ++l) {
      float* dst = (l & 1) ? h1 : h0;
      pol_layer(src, sstride, Ls[l], ws, dst, hstride, true);
      src = dst;
      sstride = hstride;
    }
    if (trunk == 0)
      pol_layer(src, sstride, Ls[N.depth], ws, lg, kPolLogitStride, false);
    else
      pol_layer(src, sstride, Ls[N.depth], ws, val, 1, false);
  }
}

// the lane's row of the input tile, as k_policy_forward builds it: (float) of the f64
// observation, the constants with the lane's alpha in alpha_col, zero beyond n_in; a row
// beyond n is zero
__device__ inline void roll_input_row(const PolNet& N, const Fc16Slot& SL, bool valid,
                                      int32_t alpha_col, double lane_alpha, float* row) {
  double o[3];
  fc16::fc16_observe(slot_state(SL), o);
  const int n_in = N.obs_len + N.n_extra;
  for (int c = 0; c < kPolInStride; ++c) {
    float v = 0.f;
    if (valid) {
      if (c < N.obs_len)
        v = (float)o[c];
      else if (c < n_in)
        v = (c - N.obs_len == alpha_col) ? (float)lane_alpha : N.extra[c - N.obs_len];
    }
    row[c] = v;
  }
}

__global__ __launch_bounds__(kPolThreads) void k_fc16_rollout_net(PolNet N, Fc16Roll R,
                                                                  int32_t hstride) {
  __shared__ int32_t hist[CPR_HIST_BINS];
  float* xin = pol_lds;
  float* ws = xin + kPolRows * kPolInStride;
  float* lg = ws + kPolNT * kPolWsStride;
  float* val = lg + kPolRows * kPolLogitStride;
  float* h0 = val + kPolRows;
  float* h1 = h0 + kPolRows * hstride;  // used from depth 2 on (policy_lds_bytes)
  const int tid = (int)threadIdx.x;
  if (tid < CPR_HIST_BINS) hist[tid] = 0;
  const bool owner = tid < kPolRows;  // the thread holds a lane
  const int64_t i = (int64_t)blockIdx.x * kPolRows + tid;
  const bool valid = owner && i < R.n;
  const int64_t n = R.n;
  fc16::Fc16Params P = R.P;
  Fc16Slot SL = {};
  double lane_alpha = 0.0, dense = 0.0;
  int64_t acts0 = 0, steps_all = 0, acts_all = 0;
  Acc acc = {};
  if (valid) {
    SL = ((const Fc16Slot*)R.slots)[i];
    if (R.lane_alpha) {
      P.t_alpha = R.lane_t[i];
      lane_alpha = R.lane_alpha[i];
      dense = R.dense_acc[i];
    }
    acts0 = R.fresh ? 0 : SL.steps + 1;
  }
  const int32_t alpha_col = R.lane_alpha ? R.alpha_col : -1;
  for (int64_t t = 0; t < R.n_steps; ++t) {
    if (owner) roll_input_row(N, SL, valid, alpha_col, lane_alpha, xin + tid * kPolInStride);
    // (pol_layer's first barrier orders the tile, and hist's zeros, before their readers)
    roll_forward(N, hstride, xin, ws, lg, val, h0, h1);
    if (valid) {
      const int64_t at = t * n + i;
      const PolChoice ch = pol_choose(lg + tid * kPolLogitStride, N.n_actions,
                                      R.deterministic != 0, [&](uint32_t* si) {
                                        *si = (uint32_t)SL.steps;
                                        return make_stream(R.seed, SL.ep);
                                      });
      if (R.action) R.action[at] = ch.action;
      if (R.logp) R.logp[at] = ch.logp;
      if (R.value) R.value[at] = (double)val[tid];
      double r;
      const bool done = slot_step(P, R.seed, SL, ch.action, &r);
      // k_policy_collect
      if (R.engine_reward) R.engine_reward[at] = r;
      const double ra = (double)SL.reward, rd = (double)(SL.progress - SL.reward),
                   prog = (double)SL.progress;
      const int64_t acts = SL.steps + 1;
      if (R.lane_alpha) {  // the gym's reward wrapper and shape (lane_env.h)
        GymStepInfo s;
        s.reward = r;
        s.done = done;
        s.era = ra;
        s.erd = rd;
        s.progress = prog;
        s.n_activations = acts;
        r = gym_reward(R.gym_reward, R.dense_target, s, &dense);
        r = shape_reward(R.reward_shape, r, lane_alpha, s);
      }
      if (R.reward) R.reward[at] = r;
      if (R.done) R.done[at] = done ? 1 : 0;
      steps_all += 1;
      if (done) {
        const double rel = (ra + rd) != 0.0 ? ra / (ra + rd) : 0.0;
        acc_episode(acc, (int64_t)__builtin_rint(ra * 1048576.0),
                    (int64_t)__builtin_rint(rd * 1048576.0),
                    (int64_t)__builtin_rint(prog * 1048576.0), rel,
                    (int64_t)(int32_t)SL.progress, SL.steps, acts, SL.status, hist);
        acts_all += acts - acts0;
        acts0 = 0;
        const uint64_t ep = SL.ep + (uint64_t)n;  // VecEnv auto-reset: the lane's next episode
        if (R.lane_alpha) {                       // k_lane_assign
          const int32_t j = lane_alpha_entry(R.schedule, R.seed, ep, R.n_alpha);
          P.t_alpha = R.tab_t[j];
          lane_alpha = R.tab_a[j];
          dense = 0.0;
        }
        slot_reset(P, R.seed, SL, ep);
      }
      if (R.lane_alpha && R.alpha) R.alpha[at] = lane_alpha;
      if (R.obs) fc16::fc16_observe(slot_state(SL), R.obs + 3 * at);
    }
  }
  // PPO's bootstrap: the value of the final observation
  if (owner) roll_input_row(N, SL, valid, alpha_col, lane_alpha, xin + tid * kPolInStride);
  roll_forward(N, hstride, xin, ws, lg, val, h0, h1);
  if (valid) {
    if (R.value) R.value[R.n_steps * n + i] = (double)val[tid];
    ((Fc16Slot*)R.slots)[i] = SL;
    if (R.lane_alpha) {
      R.lane_t[i] = P.t_alpha;
      R.lane_alpha[i] = lane_alpha;
      R.dense_acc[i] = dense;
    }
    // k_policy_tail: activations of the episode still running
    acts_all += SL.steps + 1 - acts0;
  }
  // rollout totals: every step and activation (acc holds finished episodes only)
  acc.steps = steps_all;
  acc.activations = acts_all;
  // block_flush for this workgroup's shape: the lanes sit in wave 0 alone
  if (tid < 64) {
    int64_t v[13] = {acc.episodes, acc.steps,   acc.activations,     acc.ra_fx,
                     acc.rd_fx,    acc.prog_fx, acc.orphans,         acc.tie,
                     acc.overlap,  acc.other,   (int64_t)acc.rel_fx, (int64_t)acc.rel_sq_fx,
                     acc.invalid};
    // cpr_summary word index of each accumulator (rel sums sit before orphans)
    const int idx[13] = {0, 1, 2, 3, 4, 5, 8, 9, 10, 11, 6, 7, kInvalidWord};
#pragma unroll
    for (int k = 0; k < 13; ++k) {
      const int64_t s = wave_sum(v[k]);
      if (tid == 0 && s) atomicAdd((unsigned long long*)R.sum + idx[k], (unsigned long long)s);
    }
  }
  __syncthreads();  // hist is complete
  if (tid < CPR_HIST_BINS && hist[tid])
    atomicAdd((unsigned long long*)&R.sum->hist[tid], (unsigned long long)hist[tid]);
}

static unsigned grid_of(int64_t n) { return (unsigned)((n + kBlock - 1) / kBlock); }

size_t fc16_slot_bytes() { return sizeof(Fc16Slot); }

hipError_t launch_fc16_reset(const fc16::Fc16Params& P, uint64_t seed, void* slots, int64_t n,
                             const uint8_t* mask, const uint64_t* eps, double* obs,
                             hipStream_t st, const uint64_t* lane_t) {
  if (lane_t)
    hipLaunchKernelGGL(k_fc16_reset<true>, dim3(grid_of(n)), dim3(kBlock), 0, st, P, seed,
                       (Fc16Slot*)slots, n, mask, eps, obs, lane_t);
  else
    hipLaunchKernelGGL(k_fc16_reset<false>, dim3(grid_of(n)), dim3(kBlock), 0, st, P, seed,
                       (Fc16Slot*)slots, n, mask, eps, obs, lane_t);
  return hipGetLastError();
}

hipError_t launch_fc16_step(const fc16::Fc16Params& P, uint64_t seed, void* slots, int64_t n,
                            const int32_t* actions, const StepBuffers& b, hipStream_t st,
                            const uint64_t* lane_t) {
  if (lane_t)
    hipLaunchKernelGGL(k_fc16_step<true>, dim3(grid_of(n)), dim3(kBlock), 0, st, P, seed,
                       (Fc16Slot*)slots, n, actions, b, lane_t);
  else
    hipLaunchKernelGGL(k_fc16_step<false>, dim3(grid_of(n)), dim3(kBlock), 0, st, P, seed,
                       (Fc16Slot*)slots, n, actions, b, lane_t);
  return hipGetLastError();
}

hipError_t launch_fc16_observe_fields(const void* slots, int64_t n, int32_t* f, hipStream_t st) {
  hipLaunchKernelGGL(k_fc16_observe_fields, dim3(grid_of(n)), dim3(kBlock), 0, st,
                     (const Fc16Slot*)slots, n, f);
  return hipGetLastError();
}

hipError_t launch_fc16_cursor(const void* slots, int64_t n, const LaneCursor& c, hipStream_t st) {
  hipLaunchKernelGGL(k_fc16_cursor, dim3(grid_of(n)), dim3(kBlock), 0, st,
                     (const Fc16Slot*)slots, n, c);
  return hipGetLastError();
}

static int64_t rollout_net_lds_limit() {
  return std::min<int64_t>(lds_dynamic_max((const void*)k_fc16_rollout_net),
                           160 * 1024 - 2048 - (int64_t)sizeof(int32_t) * CPR_HIST_BINS);
}

bool fc16_rollout_net_fits(const PolNet& N) {
  return policy_lds_bytes(N.depth, N.width_pi, N.width_vf) <= rollout_net_lds_limit();
}

hipError_t launch_fc16_rollout_net(const PolNet& N, const Fc16Roll& R, hipStream_t st) {
  if (R.n <= 0) return hipSuccess;
  const int64_t bytes = policy_lds_bytes(N.depth, N.width_pi, N.width_vf);
  if (bytes > rollout_net_lds_limit()) return hipErrorInvalidValue;
  CPR_LDS_GUARD(k_fc16_rollout_net, bytes);
  if (bytes > 64 * 1024) {
    const hipError_t e = hipFuncSetAttribute((const void*)k_fc16_rollout_net,
                                             hipFuncAttributeMaxDynamicSharedMemorySize,
                                             (int)rollout_net_lds_limit());
    if (e != hipSuccess) return e;
  }
  const int32_t w = N.width_pi > N.width_vf ? N.width_pi : N.width_vf;
  const int64_t blocks = (R.n + kPolRows - 1) / kPolRows;
  hipLaunchKernelGGL(k_fc16_rollout_net, dim3((unsigned)blocks), dim3(kPolThreads), (size_t)bytes,
                     st, N, R, (int32_t)policy_act_stride(w));
  return hipGetLastError();
}

hipError_t launch_fc16_episodes(const fc16::Fc16Params& P, uint64_t seed, uint64_t first,
                                int64_t n_eps, int64_t lanes, cpr_episode_record* recs,
                                cpr_summary* sum, hipStream_t st) {
  const unsigned blocks = (unsigned)(lanes / kBlock);
  hipLaunchKernelGGL(k_fc16_episodes, dim3(blocks), dim3(kBlock), 0, st, P,
                     SeedSource{seed, first}, n_eps, recs, sum);
  return hipGetLastError();
}

}  // namespace cpr
