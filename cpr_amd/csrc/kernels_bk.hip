// B_k kernels for gfx950: one lane = one episode / gym env of the bk_ssz attack space,
// driven by the exact per-lane event engine of bk_lane.h. Each lane owns one contiguous
// HBM region (vertex ring, per-node visibility and times, quorums, drafts, event heap,
// scratch) reused for every episode it runs.
//
// This unit holds what is B_k's own: the adapter (BkAdapter: slot, head rewards, observation
// encodings, slab hooks), the policy decode kernel, and the kernel shells with their names,
// occupancy and slab symbol. The kernel bodies and the launchers are ev_kernels.h's, shared
// with kernels_eth.hip and kernels_ts.hip, except k_bk_run_episodes, which keeps a body of its
// own (measured slower as a shell, see the kernel):
//
//   k_bk_run_episodes  fused reset/(policy, step)* episodes, or Simulator.loop tasks
//   k_bk_reset/k_bk_step  lockstep gym API (engine.ml reset / step) with host actions
//   k_bk_rollout       lockstep rollout on the device (BASELINE configs[4])
#include <hip/hip_runtime.h>

#include "../../include/cpr_hip.h"
#include "bk_lane.h"
#include "ev_kernels.h"

#pragma clang fp contract(off)

namespace cpr {

struct BkSlot {
  bk::BkLane L;
  uint64_t ep;
  double last_ra;
  int32_t head;
  int32_t live;
};

// ev_kernels.h / wave_sched.h adapter for bk_lane.h
struct BkAdapter : EvAdapterBase<bk::BkLane, bk::BkParams, bk::BkMem> {
  using Slot = BkSlot;
  using Obs = bk::BkObs;
  static constexpr int kObs = 8;
  static constexpr bool kSlab = true, kRollSched = true;
  static constexpr int kEvLpw = 64, kRollLpw = 0;

  __device__ static bool pow0(uint32_t ev) {
    return (ev & 7u) == bk::EV_DAG && (ev >> 5) == 0u && ((ev >> 3) & 3u) == bk::KD_POW;
  }
  template <class St>
  __device__ __forceinline__ static void run_pow0(Lane& L, const Par& P, const St& S,
                                                  const Mem& M, int32_t) {
    const int32_t v = L.append_vote(P, S, M, 0, L.priv);
    L.push_now(P, M, bk::mkev(bk::EV_MV, 0, bk::KD_POW), v);
  }
  __device__ __forceinline__ static Obs observe(Lane& L, const Par& P, const Mem& M) {
    return L.observe(P, M);
  }
  __device__ __forceinline__ static int32_t policy(Lane& L, const Par& P, const Mem& M) {
    return bk::bk_policy(P, L.observe(P, M));
  }
  __device__ static void act(Lane& L, const Par& P, const Mem& M) {
    L.apply(P, M, policy(L, P, M));
    ++L.steps;
  }
  __device__ static int32_t head_gym(Lane& L, const Par& P, const Mem& M, int32_t att) {
    return L.head(P, M, att);
  }
  __device__ static int32_t head_loop(Lane& L, const Par& P, const Mem& M) {
    return L.head(P, M, P.net == 2 ? M.tips[0] : L.priv);
  }
  __device__ static bool gym_done(Lane& L, const Par& P, const Mem& M, int32_t hd) {
    const double progress = (double)(L.X(P, M, hd).height * P.k);
    return L.dead || !(L.steps < P.max_steps && progress < P.max_progress && L.now < P.max_time);
  }

  __host__ __device__ static int64_t lane_bytes(const Par& P) { return bk::bk_lane_bytes(P); }
  __device__ __forceinline__ static Mem mem_at(uint8_t* base, const Par& P) {
    return bk::bk_mem_at(base, P);
  }
  __device__ __forceinline__ static void node_mem(Mem& M, uint8_t* base, const Par& P) {
    bk::bk_node_mem(M, base, P);
  }
  __device__ __forceinline__ static void slab_attach(Mem& M, const SlabView& s, int32_t col,
                                                     int32_t cols) {
    bk::bk_heap_slab(M, s.base, col, cols, s.kl);
    bk::bk_vis_window(M, (uint8_t*)(s.base + (size_t)s.kl * cols), col, s.vw);
  }
  __device__ __forceinline__ static void slab_load(const Mem& M, const Par& P, const Lane& L) {
    bk::bk_heap_load(M, L.hused);
    bk::bk_vis_load(M, P, L.newest);
  }
  __device__ __forceinline__ static void slab_store(const Mem& M, const Lane& L) {
    bk::bk_heap_store(M, L.hused);
  }
  __device__ __forceinline__ static void slot_head(Slot& SL, int32_t hd) { SL.head = hd; }

  // the head's rewards are its int vertex fields
  __device__ __forceinline__ static const bk::BVtx& head_at(Lane& L, const Par& P, const Mem& M,
                                                            int32_t hd) {
    return L.X(P, M, hd);
  }
  __device__ __forceinline__ static double reward_att(Lane&, const Par&, const Mem&,
                                                      const bk::BVtx& h) {
    return (double)h.rew_att;
  }
  __device__ __forceinline__ static EvHead head(Lane&, const Par& P, const Mem&,
                                                const bk::BVtx& h) {
    return {(double)h.rew_att, (double)h.rew_def, (double)(h.height * P.k), h.time, h.height,
            h.who, 0};
  }
  __device__ __forceinline__ static int32_t miner(const bk::BVtx& h) { return h.who; }
  __device__ __forceinline__ static void acc(Acc& acc, const Par& P, Lane& L, const Mem&,
                                             const bk::BVtx& h, int32_t* hist) {
    const int32_t ra = h.rew_att, rd = h.rew_def;
    const double rel = (ra + rd) != 0 ? (double)ra / (double)(ra + rd) : 0.0;
    // orphans: activations (votes) not confirmed by the head's chain
    acc_episode(acc, (int64_t)ra << 20, (int64_t)rd << 20, (int64_t)h.height * P.k << 20, rel,
                (int64_t)h.height * P.k, L.steps, L.c_act, L.status, hist);
  }
  __device__ __forceinline__ static auto node_rews(Lane&, const Par& P, const Mem& M, int32_t,
                                                   const bk::BVtx& h) {
    const int32_t* hr =
        h.qslot < 0 ? nullptr : M.nrew + (int64_t)(h.qslot & (P.cap_q - 1)) * P.n;
    return [hr](int32_t j) { return hr ? (double)hr[j] : 0.0; };
  }

  __device__ __forceinline__ static void fields(const Obs& o, int32_t* g) {
    g[0] = o.public_blocks;
    g[1] = o.private_blocks;
    g[2] = o.diff_blocks;
    g[3] = o.public_votes;
    g[4] = o.private_votes_inclusive;
    g[5] = o.private_votes_exclusive;
    g[6] = o.lead;
    g[7] = o.event;
  }
  // ssz_tools.ml:1-74 with bk_ssz.ml:37-48 normalizers; unit encodings use host-tabulated
  // libm values (tabs = [2/pi atan(i) | 0.5 + atan(i - N)/pi | 2/pi atan(i/k)], i < N)
  __device__ __forceinline__ static void write_obs(const Par& P, const Obs& o, int unit,
                                                   const double* tabs, int32_t tn, double* out) {
    const double pi = 3.141592653589793;
    const int32_t k = P.k;
    if (!unit) {
      out[0] = (double)o.public_blocks;
      out[1] = (double)o.private_blocks;
      out[2] = (double)o.diff_blocks;
      out[3] = (double)o.public_votes;
      out[4] = (double)o.private_votes_inclusive;
      out[5] = (double)o.private_votes_exclusive;
      out[6] = o.lead ? 1.0 : 0.0;
      out[7] = (double)o.event;
      return;
    }
    auto nn1 = [&](int32_t x) { return x < tn ? tabs[x] : 2.0 / pi * atan((double)x / 1.0); };
    auto nnk = [&](int32_t x) {
      return x < tn ? tabs[3 * tn + x] : 2.0 / pi * atan((double)x / (double)k);
    };
    out[0] = nn1(o.public_blocks);
    out[1] = nn1(o.private_blocks);
    const int32_t d = o.diff_blocks;
    out[2] = (d > -tn && d < tn) ? tabs[tn + d + tn] : 0.5 + (1.0 / pi * atan((double)d / 1.0));
    out[3] = nnk(o.public_votes);
    out[4] = nnk(o.private_votes_inclusive);
    out[5] = nnk(o.private_votes_exclusive);
    out[6] = o.lead ? 1.0 : 0.0;
    out[7] = (double)o.event / 2.0;
  }

  // the kernels' parameters after the shared ones
  static auto fused_tail(const EvSlab& sl, int32_t) { return std::make_tuple(sl.kl, sl.vw); }
  static auto roll_tail(const EvSlab& sl, int32_t lpw) {
    return std::make_tuple(sl.kl, sl.vw, lpw);
  }
};

// k_bk_run_episodes' own finish (see the kernel)
__device__ inline void bk_acc(Acc& acc, const bk::BkParams& P, const bk::BkLane& L,
                              const bk::BVtx& h, int32_t* hist) {
  const int32_t ra = h.rew_att, rd = h.rew_def;
  const double rel = (ra + rd) != 0 ? (double)ra / (double)(ra + rd) : 0.0;
  // orphans: activations (votes) not confirmed by the head's chain
  acc_episode(acc, (int64_t)ra << 20, (int64_t)rd << 20, (int64_t)h.height * P.k << 20, rel,
              (int64_t)h.height * P.k, L.steps, L.c_act, L.status, hist);
}

// one finished episode: summary, record, per-node row
template <class Src, class St>
__device__ inline void bk_finish(const bk::BkParams& P, bk::BkLane& L, const bk::BkMem& M,
                                 const St& S, int64_t e, int32_t hd, Acc& acc, int32_t* hist,
                                 cpr_episode_record* recs, const NodeOut& no) {
  L.status |= Src::missed(S);
  const bk::BVtx& h = L.X(P, M, hd);
  bk_acc(acc, P, L, h, hist);
  if (recs) {
    cpr_episode_record r;
    r.reward_attacker = (double)h.rew_att;
    r.reward_defender = (double)h.rew_def;
    r.progress = (double)(h.height * P.k);
    r.chain_time = h.time;
    r.sim_time = P.mode == CPR_MODE_GYM ? L.now : 0.0;
    r.n_steps = L.steps;
    r.n_activations = L.c_act;
    r.head_height = h.height;
    r.head_miner = h.who;
    r.status = L.status;
    r.head_work = 0;
    recs[e] = r;
  }
  if (no.acts) {  // csv_runner.ml:74-79: sim.activations and (Dag.data head).rewards
    const int32_t* hr =
        h.qslot < 0 ? nullptr : M.nrew + (int64_t)(h.qslot & (P.cap_q - 1)) * P.n;
    for (int32_t j = 0; j < P.n; ++j) {
      no.acts[e * P.n + j] = M.nact[j];
      no.rews[e * P.n + j] = hr ? (double)hr[j] : 0.0;
    }
    no.head_miner[e] = h.who;
  }
}

// the heap slab of a workgroup (dynamic LDS): kl nodes per lane, node-major
extern __shared__ __attribute__((aligned(16))) bk::HNode bk_slab[];

template <class Src>
__global__ __launch_bounds__(kBlock) CPR_EV_OCC void k_bk_run_episodes(
    bk::BkParams P, Src src, int64_t n_eps, uint8_t* mem, int64_t lane_bytes,
    cpr_episode_record* recs, cpr_summary* sum, NodeOut no, int32_t kl, int32_t vw) {
  // B_k's own copy of ev_run_episodes_body: as a shell around the shared body the kernel
  // compiled to other registers (236 VGPRs against 243) and measured 0.65 % slower on the
  // 2048-step minor-delay probe (DESIGN.md §5 "One body per event-engine kernel")
  __shared__ int32_t hist[CPR_HIST_BINS];
  if (threadIdx.x < CPR_HIST_BINS) hist[threadIdx.x] = 0;
  __syncthreads();
  const int64_t tid = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int64_t nthreads = (int64_t)gridDim.x * blockDim.x;
  bk::BkMem M = bk::bk_mem_at(mem + tid * lane_bytes, P);
  // every episode starts with an empty heap and a fresh window (init): the slab needs no
  // load or store
  bk::bk_heap_slab(M, bk_slab, (int32_t)threadIdx.x, (int32_t)blockDim.x, kl);
  bk::bk_vis_window(M, (uint8_t*)(bk_slab + (size_t)kl * blockDim.x), (int32_t)threadIdx.x, vw);
  if (no.mem) bk::bk_node_mem(M, no.mem + tid * no.lane_bytes, P);
  Acc acc = {};
  bk::BkLane L;
#if CPR_EV_SCHED
  int64_t e = tid;  // wave-coherent dispatch (wave_sched.h), episodes from a work queue
  auto S = src.at(e < n_eps ? e : 0);
  EvCursor c;
  c.cls = -1;
  c.phase = PH_IDLE;
  if (e < n_eps) ev_begin<BkAdapter>(L, P, S, M, c);
  for (;;) {
    while (c.phase != PH_IDLE && c.cls < 0) {
      if (c.phase != PH_OVER) ev_fetch<BkAdapter>(L, P, S, M, c);
      if (c.phase == PH_OVER) {
        bk_finish<Src>(P, L, M, S, e, c.hd, acc, hist, recs, no);
        e = ev_next_episode(P.next, e, nthreads);
        if (e < n_eps) {
          S = src.at(e);
          ev_begin<BkAdapter>(L, P, S, M, c);
        } else {
          c.phase = PH_IDLE;
        }
      }
    }
    const int32_t k = ev_choose(c.cls);
    if (k < 0) break;
    if (c.cls == k) ev_exec<BkAdapter>(L, P, S, M, c);
  }
#else
  for (int64_t e = tid; e < n_eps; e += nthreads) {
    const auto S = src.at(e);
    int32_t hd;
    if (P.mode == CPR_MODE_GYM) {
      L.gym_reset(P, S, M);
      bool done = L.dead != 0;
      hd = 0;
      while (!done) hd = L.gym_step(P, S, M, BkAdapter::policy(L, P, M), &done);
    } else {
      hd = L.loop(P, S, M);
    }
    bk_finish<Src>(P, L, M, S, e, hd, acc, hist, recs, no);
  }
#endif
  __syncthreads();
  block_flush(acc, hist, sum);
}

template <bool LT>
__global__ __launch_bounds__(kBlock) void k_bk_reset(
    bk::BkParams P, uint64_t seed, uint8_t* mem, int64_t lane_bytes, BkSlot* slots, int64_t n,
    const uint8_t* mask, const uint64_t* eps, int unit, const double* tabs, int32_t tn, double* obs,
    const uint64_t* lane_t) {
  ev_reset_body<BkAdapter, LT>(P, seed, mem, lane_bytes, slots, n, mask, eps, unit, tabs, tn,
                               obs, lane_t);
}

template <bool LT>
__global__ __launch_bounds__(kBlock) void k_bk_step(
    bk::BkParams P, uint64_t seed, uint8_t* mem, int64_t lane_bytes, BkSlot* slots, int64_t n,
    const int32_t* actions, int unit, const double* tabs, int32_t tn, StepBuffers out,
    const uint64_t* lane_t) {
  ev_step_body<BkAdapter, LT>(P, seed, mem, lane_bytes, slots, n, actions, unit, tabs, tn, out,
                              lane_t);
}

// four waves per SIMD (128 VGPRs): rollout_lanes_per_wave spreads a small batch over them
#ifndef CPR_ROLL_WAVES
#define CPR_ROLL_WAVES 4
#endif
#if CPR_EV_WAVES > 0
#define CPR_ROLL_OCC CPR_EV_OCC
#else
#define CPR_ROLL_OCC __attribute__((amdgpu_waves_per_eu(CPR_ROLL_WAVES)))
#endif
__global__ __launch_bounds__(kBlock) CPR_ROLL_OCC void k_bk_rollout(
    bk::BkParams P, uint64_t seed, uint8_t* mem, int64_t lane_bytes, BkSlot* slots, int64_t n,
    int64_t n_steps, int unit, const double* tabs, int32_t tn, double* obs, double* reward,
    uint8_t* done_out, cpr_summary* sum, int32_t kl, int32_t vw, int32_t lpw) {
  ev_rollout_body<BkAdapter>(P, seed, mem, lane_bytes, slots, n, n_steps, unit, tabs, tn, obs,
                             reward, done_out, sum, SlabView{bk_slab, kl, vw, 0, 0}, lpw);
}

__global__ void k_bk_observe_fields(
    bk::BkParams P, uint8_t* mem, int64_t lane_bytes, const BkSlot* slots, int64_t n, int32_t* f) {
  ev_observe_fields_body<BkAdapter>(P, mem, lane_bytes, slots, n, f);
}

// engine.ml:258-261: decode (ssz_tools.ml:42-58 of_float) and apply the policy
__global__ void k_bk_policy(bk::BkParams P, int unit, const double* obs, int64_t n,
                            int32_t* actions) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const double* x = obs + 8 * i;
  const double pi = 3.141592653589793;
  int32_t v[8];
  for (int j = 0; j < 8; ++j) {
    if (j == 6) {
      v[j] = x[j] >= 0.5 ? 1 : 0;
    } else if (j == 7) {
      v[j] = unit ? (int32_t)floor(x[j] * 2.0) : (int32_t)x[j];
    } else if (!unit) {
      v[j] = (int32_t)x[j];
    } else {
      const double scale = j >= 3 ? (double)P.k : 1.0;
      v[j] = j == 2 ? (int32_t)__builtin_round(tan(pi * (x[j] - 0.5)) * scale)
                    : (int32_t)__builtin_round(tan(pi / 2.0 * x[j]) * scale);
    }
  }
  const bk::BkObs o{v[0], v[1], v[2], v[3], v[4], v[5], v[6], v[7]};
  actions[i] = bk::bk_policy(P, o);
}

// ---------------------------------------------------------------- launchers

hipError_t launch_bk_run_episodes(const bk::BkParams& P, uint64_t seed, uint64_t first,
                                  int64_t n_eps, uint8_t* mem, int64_t lane_bytes, int64_t lanes,
                                  cpr_episode_record* recs, cpr_summary* sum, hipStream_t st,
                                  const NodeOut& no) {
  return ev_launch_episodes<BkAdapter>(k_bk_run_episodes<SeedSource>, P, SeedSource{seed, first},
                                       n_eps, mem, lane_bytes, lanes, recs, sum, st, no);
}

hipError_t launch_bk_replay_episodes(const bk::BkParams& P, const TraceSource& src, int64_t n_eps,
                                 uint8_t* mem, int64_t lane_bytes, int64_t lanes,
                                 cpr_episode_record* recs, cpr_summary* sum, hipStream_t st,
                                  const NodeOut& no) {
  return ev_launch_episodes<BkAdapter>(k_bk_run_episodes<TraceSource>, P, src, n_eps, mem,
                                       lane_bytes, lanes, recs, sum, st, no);
}

hipError_t launch_bk_reset(const bk::BkParams& P, uint64_t seed, uint8_t* mem, int64_t lane_bytes,
                           void* slots, int64_t n, const uint8_t* mask, const uint64_t* eps,
                           int unit, const double* tabs, int32_t tn, double* obs,
                           hipStream_t st, const uint64_t* lane_t) {
  return ev_launch_lanes<BkAdapter>(lane_t ? k_bk_reset<true> : k_bk_reset<false>, lane_bytes, n,
                                    st, P, seed, mem, lane_bytes, (BkSlot*)slots, n, mask, eps,
                                    unit, tabs, tn, obs, lane_t);
}

hipError_t launch_bk_step(const bk::BkParams& P, uint64_t seed, uint8_t* mem, int64_t lane_bytes,
                          void* slots, int64_t n, const int32_t* actions, int unit,
                          const double* tabs, int32_t tn, const StepBuffers& b, hipStream_t st,
                          const uint64_t* lane_t) {
  return ev_launch_lanes<BkAdapter>(lane_t ? k_bk_step<true> : k_bk_step<false>, lane_bytes, n, st,
                                    P, seed, mem, lane_bytes, (BkSlot*)slots, n, actions, unit,
                                    tabs, tn, b, lane_t);
}

hipError_t launch_bk_rollout(const bk::BkParams& P, uint64_t seed, uint8_t* mem,
                             int64_t lane_bytes, void* slots, int64_t n, int64_t n_steps,
                             int unit, const double* tabs, int32_t tn, double* obs,
                             double* reward, uint8_t* done, cpr_summary* sum, hipStream_t st) {
  return ev_launch_rollout<BkAdapter>(k_bk_rollout, P, seed, mem, lane_bytes, slots, n, n_steps,
                                      unit, tabs, tn, obs, reward, done, sum, st);
}

hipError_t launch_bk_observe_fields(const bk::BkParams& P, uint8_t* mem, int64_t lane_bytes,
                                    const void* slots, int64_t n, int32_t* f, hipStream_t st) {
  return ev_launch_lanes<BkAdapter>(k_bk_observe_fields, lane_bytes, n, st, P, mem, lane_bytes,
                                    (const BkSlot*)slots, n, f);
}

hipError_t launch_bk_cursor(const void* slots, int64_t n, const LaneCursor& c, hipStream_t st) {
  return ev_launch_cursor<BkAdapter>(slots, n, c, st);
}

hipError_t launch_bk_policy(const bk::BkParams& P, int unit, const double* obs, int64_t n,
                            int32_t* actions, hipStream_t st) {
  hipLaunchKernelGGL(k_bk_policy, dim3(grid_of(n)), dim3(kBlock), 0, st, P, unit, obs, n,
                     actions);
  return hipGetLastError();
}

size_t bk_slot_bytes() { return sizeof(BkSlot); }

int bk_blocks_per_cu() { return ev_blocks_per_cu(k_bk_run_episodes<SeedSource>); }

}  // namespace cpr
