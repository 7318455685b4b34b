// gfx950 kernels of the neural-network policy (policy_net.h):
//   k_policy_forward   the whole actor-critic MLP for a tile of rows per workgroup, on the
//                      f32-input MFMA (v_mfma_f32_16x16x4_f32: f32 in, f32 accumulate), then
//                      argmax / keyed sampling, log-probability and value per row in f64
//   k_policy_collect   per-step bookkeeping of cpr_rollout_net: step-major outputs (with a
//                      lane env the gym's wrapped and shaped reward, lane_env.h), summary
//                      of finished episodes, lane cursors, reset mask
//   k_lane_assign      the lane env's assumption schedule: threshold and alpha of the masked
//                      lanes' new episodes, before every lockstep reset
//   k_policy_tail      activations of the episodes still running when the rollout ends
//   k_eval_collect     per-step bookkeeping of cpr_eval_net: the episode's reward summed per
//                      lane, one cpr_eval_record per finished episode of the set at a
//                      deterministic slot, the finished-episode counter
//   k_eval_reduce      after the evaluation, one workgroup per alpha: its cpr_summary and the
//                      mean / std of the logged columns in eval.h's order
//   k_lock_cursor      where the Nakamoto lockstep lanes stand when a rollout begins
#include <hip/hip_runtime.h>

#include <algorithm>

#include "eval.h"
#include "kernels.h"
#include "lane_env.h"
#include "nak_rollout.h"
#include "policy_layer.h"
#include "policy_net.h"
#include "summary.h"

#pragma clang fp contract(off)

namespace cpr {

__global__ __launch_bounds__(kPolThreads) void k_policy_forward(PolNet N, PolIO io, int32_t hstride) {
  float* xin = pol_lds;
  float* ws = xin + kPolRows * kPolInStride;
  float* lg = ws + kPolNT * kPolWsStride;
  float* val = lg + kPolRows * kPolLogitStride;
  float* h0 = val + kPolRows;
  float* h1 = h0 + kPolRows * hstride;  // used from depth 2 on (policy_lds_bytes)
  const int tid = (int)threadIdx.x;
  const int64_t r0 = (int64_t)blockIdx.x * kPolRows;
  const int n_in = N.obs_len + N.n_extra;
  // the input tile: f64 observation -> f32, the batch constants appended, zero beyond n_in
  // and for rows beyond n
  for (int idx = tid; idx < kPolRows * kPolInStride; idx += kPolThreads) {
    const int r = idx / kPolInStride, c = idx - r * kPolInStride;
    const int64_t row = r0 + r;
    float v = 0.f;
    if (row < io.n) {
      if (c < N.obs_len)
        v = (float)io.obs[row * N.obs_len + c];
      else if (c < n_in)
        v = (io.lane_alpha && c - N.obs_len == io.alpha_col) ? (float)io.lane_alpha[row]
                                                             : N.extra[c - N.obs_len];
    }
    xin[idx] = v;
  }
  // (pol_layer's first barrier orders the tile before its readers)
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
  const int64_t row = r0 + tid;
  if (tid >= kPolRows || row >= io.n) return;
  const float* l = lg + tid * kPolLogitStride;
  const int na = N.n_actions;
  const PolChoice ch = pol_choose(l, na, io.deterministic != 0, [&](uint32_t* si) {
    const uint64_t ep = io.ep ? io.ep[row] : io.episode0 + (uint64_t)row;
    *si = io.step ? (uint32_t)io.step[row] : 0u;
    return make_stream(io.seed, ep);
  });
  if (io.action) io.action[row] = ch.action;
  if (io.logp) io.logp[row] = ch.logp;
  if (io.value) io.value[row] = (double)val[tid];
  if (io.logits)
    for (int i = 0; i < na; ++i) io.logits[row * na + i] = l[i];
}

__global__ __launch_bounds__(kBlock) void k_policy_collect(PolCollect C, int64_t n) {
  __shared__ int32_t hist[CPR_HIST_BINS];
  if (threadIdx.x < CPR_HIST_BINS) hist[threadIdx.x] = 0;
  __syncthreads();
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  Acc acc = {};
  int64_t steps_all = 0, acts_all = 0;
  if (i < n) {
    const uint8_t d = C.done[i];
    double r = C.reward[i];
    if (C.out_engine_reward) C.out_engine_reward[i] = r;
    if (C.lane_alpha) {  // the gym's reward wrapper and shape (lane_env.h)
      GymStepInfo s;
      s.reward = r;
      s.done = d != 0;
      s.era = C.era[i];
      s.erd = C.erd[i];
      s.progress = C.eprog[i];
      s.n_activations = C.eacts[i];
      double acc = C.dense_acc[i];
      r = gym_reward(C.gym_reward, C.dense_target, s, &acc);
      if (C.gym_reward == CPR_GYM_REWARD_DENSE_PER_PROGRESS) C.dense_acc[i] = acc;
      r = shape_reward(C.reward_shape, r, C.lane_alpha[i], s);
    }
    if (C.out_reward) C.out_reward[i] = r;
    if (C.out_done) C.out_done[i] = d;
    C.mask[i] = d;
    steps_all = 1;
    if (d) {
      // summary.h's fixed-point rule on the step infos of the episode's last step
      const double ra = C.era[i], rd = C.erd[i], prog = C.eprog[i];
      const double rel = (ra + rd) != 0.0 ? ra / (ra + rd) : 0.0;
      const int64_t acts = C.eacts[i];
      const int64_t hh = C.orphans_from_progress ? (int64_t)prog : (int64_t)C.hh[i];
      acc_episode(acc, (int64_t)__builtin_rint(ra * 1048576.0),
                  (int64_t)__builtin_rint(rd * 1048576.0),
                  (int64_t)__builtin_rint(prog * 1048576.0), rel, hh, C.esteps[i], acts,
                  C.status[i], hist);
      acts_all = acts - C.acts0[i];
      C.acts0[i] = 0;
      C.ep[i] += (uint64_t)n;  // VecEnv auto-reset: the lane's next episode
      C.step[i] = 0;
    } else {
      C.step[i] += 1;
    }
  }
  // rollout totals: every step and activation (acc holds finished episodes only)
  acc.steps = steps_all;
  acc.activations = acts_all;
  __syncthreads();
  block_flush(acc, hist, C.sum);
}

__global__ __launch_bounds__(kBlock) void k_policy_tail(const int64_t* acts, const int64_t* acts0,
                                                        int64_t n, cpr_summary* sum) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int64_t v = wave_sum(i < n ? acts[i] - acts0[i] : 0);
  if ((threadIdx.x & 63) == 0 && v)
    atomicAdd((unsigned long long*)&sum->activations, (unsigned long long)v);
}

__global__ __launch_bounds__(kBlock) void k_eval_collect(EvalCollect C, int64_t n) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  int64_t fin = 0;
  if (i < n) {
    const uint8_t d = C.done[i];
    double r = C.reward[i];
    double alpha = C.cfg_alpha;
    if (C.lane_alpha) {  // the gym's reward wrapper and shape (lane_env.h), as k_policy_collect
      GymStepInfo s;
      s.reward = r;
      s.done = d != 0;
      s.era = C.era[i];
      s.erd = C.erd[i];
      s.progress = C.eprog[i];
      s.n_activations = C.eacts[i];
      alpha = C.lane_alpha[i];
      double acc = C.dense_acc[i];
      r = gym_reward(C.gym_reward, C.dense_target, s, &acc);
      if (C.gym_reward == CPR_GYM_REWARD_DENSE_PER_PROGRESS) C.dense_acc[i] = acc;
      r = shape_reward(C.reward_shape, r, alpha, s);
    }
    const double total = C.ep_reward[i] + r;  // erw_episode_reward, in step order from 0
    C.mask[i] = d;
    if (d) {
      const uint64_t e = C.ep[i];
      const uint64_t slot = e - C.first;
      if (e >= C.first && slot < (uint64_t)C.n_set) {
        const double prog = C.eprog[i];
        cpr_eval_record rec;
        rec.episode = e;
        rec.alpha = alpha;
        rec.episode_reward = total;
        rec.episode_sim_time = C.est[i];
        rec.episode_chain_time = C.ect[i];
        rec.episode_progress = prog;
        rec.reward_attacker = C.era[i];
        rec.reward_defender = C.erd[i];
        rec.episode_n_activations = C.eacts[i];
        rec.episode_n_steps = C.esteps[i];
        rec.height = C.orphans_from_progress ? (int64_t)prog : (int64_t)C.hh[i];
        rec.alpha_index =
            C.lane_alpha ? lane_alpha_entry(C.schedule, C.seed, e, C.n_alpha) : 0;
        rec.status = C.status[i];
        C.records[slot] = rec;
        fin = 1;
      }
      C.ep_reward[i] = 0.0;
      C.ep[i] = e + (uint64_t)n;  // VecEnv auto-reset: the lane's next episode
      C.step[i] = 0;
    } else {
      C.ep_reward[i] = total;
      C.step[i] += 1;
    }
  }
  // every lane of the wave takes part in the shuffle: one atomic per wave that finished any
  fin = wave_sum(fin);
  if ((threadIdx.x & 63) == 0 && fin) atomicAdd(C.finished, (unsigned long long)fin);
}

static_assert(kEvalThreads == kBlock, "block_flush reduces a workgroup of kBlock threads");

__global__ __launch_bounds__(kEvalThreads) void k_eval_reduce(EvalReduce R) {
  __shared__ int32_t hist[CPR_HIST_BINS];
  __shared__ double p[kEvalThreads];
  __shared__ unsigned long long n_valid;
  const int t = (int)threadIdx.x;
  const int32_t j = (int32_t)blockIdx.x;  // the table entry
  const uint64_t A = (uint64_t)R.n_alpha;
  // the first slot s with (first + s) mod A = j; the entry's records follow at stride A
  const int64_t s0 = (int64_t)(((uint64_t)j + A - R.first % A) % A);
  const cpr_eval_record* recs = R.records + s0;
  const int64_t stride = (int64_t)A, count = R.per_alpha;
  if (t < CPR_HIST_BINS) hist[t] = 0;
  if (t == 0) n_valid = 0ull;
  __syncthreads();
  Acc acc = {};
  for (int64_t k = t; k < count; k += kEvalThreads) {
    const EvalTerms T = eval_terms(recs[k * stride]);
    acc_episode(acc, T.ra_fx, T.rd_fx, T.prog_fx, T.rel, T.height, T.steps, T.acts, T.status,
                hist);
  }
  if (acc.episodes) atomicAdd(&n_valid, (unsigned long long)acc.episodes);
  __syncthreads();
  block_flush(acc, hist, &R.sums[j]);
  const int64_t nv = (int64_t)n_valid;
  cpr_eval_alpha* out = &R.out[j];
  if (t == 0) {
    out->alpha = R.tab_a ? R.tab_a[j] : R.cfg_alpha;
    out->n = nv;
  }
  for (int c = 0; c < CPR_EVAL_COLUMNS; ++c) {
    double mean = 0.0;
    for (int pass = 0; pass < 2; ++pass) {
      __syncthreads();  // p's readers of the previous round are done
      p[t] = eval_partial(recs, stride, count, t, c, pass == 1, mean);
      __syncthreads();
      for (int off = kEvalThreads / 2; off > 0; off >>= 1) {
        eval_tree_level(p, t, off);
        __syncthreads();
      }
      if (pass == 0)
        mean = eval_mean(p[0], nv);
      else if (t == 0)
        out->std[c] = eval_std(p[0], nv);
    }
    if (t == 0) out->mean[c] = mean;
  }
}

__global__ __launch_bounds__(kBlock) void k_lane_assign(LaneAssign A, int64_t n) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  if (A.mask == nullptr || A.mask[i]) {
    const uint64_t ep = A.eps ? A.eps[i] : (uint64_t)i;
    const int32_t j = lane_alpha_entry(A.schedule, A.seed, ep, A.n_alpha);
    A.lane_t[i] = A.tab_t[j];
    A.lane_alpha[i] = A.tab_a[j];
    A.dense_acc[i] = 0.0;
  }
  if (A.out_alpha) A.out_alpha[i] = A.lane_alpha[i];
}

// LaneCursor of the Nakamoto lockstep lanes (closed form, or the lane's exact-engine slot)
__global__ void k_lock_cursor(LockBuffers B, int64_t n, LaneCursor c) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const LockLane& LL = ((const LockLane*)B.lanes)[i];
  const bool live = LL.live != 0;
  c.ep[i] = live ? LL.ep : (uint64_t)i;
  c.steps[i] = live ? LL.steps : 0;
  int64_t acts = live ? (int64_t)LL.L.k : 0;
  if (live && LL.exact) acts = ((const eth::EthLane*)B.eslots)[LL.exact - 1].c_act;
  c.acts[i] = acts;
}

// ---------------------------------------------------------------- launchers

hipError_t launch_lock_cursor(const LockBuffers& B, int64_t n, const LaneCursor& c,
                              hipStream_t st) {
  hipLaunchKernelGGL(k_lock_cursor, dim3((unsigned)((n + kBlock - 1) / kBlock)), dim3(kBlock), 0,
                     st, B, n, c);
  return hipGetLastError();
}

int64_t policy_lds_limit() {
  return std::min<int64_t>(lds_dynamic_max((const void*)k_policy_forward), 160 * 1024 - 2048);
}

hipError_t launch_policy_forward(const PolNet& N, const PolIO& io, hipStream_t st) {
  if (io.n <= 0) return hipSuccess;
  const int64_t bytes = policy_lds_bytes(N.depth, N.width_pi, N.width_vf);
  if (bytes > policy_lds_limit()) return hipErrorInvalidValue;
  CPR_LDS_GUARD(k_policy_forward, bytes);
  if (bytes > 64 * 1024) {
    const hipError_t e = hipFuncSetAttribute((const void*)k_policy_forward,
                                             hipFuncAttributeMaxDynamicSharedMemorySize,
                                             (int)policy_lds_limit());
    if (e != hipSuccess) return e;
  }
  const int32_t w = N.width_pi > N.width_vf ? N.width_pi : N.width_vf;
  const int64_t blocks = (io.n + kPolRows - 1) / kPolRows;
  hipLaunchKernelGGL(k_policy_forward, dim3((unsigned)blocks), dim3(kPolThreads), (size_t)bytes, st, N,
                     io, (int32_t)policy_act_stride(w));
  return hipGetLastError();
}

hipError_t launch_policy_collect(const PolCollect& C, int64_t n, hipStream_t st) {
  hipLaunchKernelGGL(k_policy_collect, dim3((unsigned)((n + kBlock - 1) / kBlock)), dim3(kBlock), 0,
                     st, C, n);
  return hipGetLastError();
}

hipError_t launch_lane_assign(const LaneAssign& A, int64_t n, hipStream_t st) {
  hipLaunchKernelGGL(k_lane_assign, dim3((unsigned)((n + kBlock - 1) / kBlock)), dim3(kBlock), 0,
                     st, A, n);
  return hipGetLastError();
}

hipError_t launch_eval_collect(const EvalCollect& C, int64_t n, hipStream_t st) {
  hipLaunchKernelGGL(k_eval_collect, dim3((unsigned)((n + kBlock - 1) / kBlock)), dim3(kBlock), 0,
                     st, C, n);
  return hipGetLastError();
}

hipError_t launch_eval_reduce(const EvalReduce& R, hipStream_t st) {
  hipLaunchKernelGGL(k_eval_reduce, dim3((unsigned)R.n_alpha), dim3(kEvalThreads), 0, st, R);
  return hipGetLastError();
}

hipError_t launch_policy_tail(const int64_t* acts, const int64_t* acts0, int64_t n,
                              cpr_summary* sum, hipStream_t st) {
  hipLaunchKernelGGL(k_policy_tail, dim3((unsigned)((n + kBlock - 1) / kBlock)), dim3(kBlock), 0,
                     st, acts, acts0, n, sum);
  return hipGetLastError();
}

}  // namespace cpr
