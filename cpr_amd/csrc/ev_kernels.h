// The kernels around the per-lane event engines (bk_lane.h, ethereum_lane.h, ts_lane.h),
// written once over the per-protocol adapter A that wave_sched.h already drives:
//
//   ev_run_episodes_body   fused reset/(policy, step)* episodes, or Simulator.loop tasks
//   ev_reset_body / ev_step_body   lockstep gym API (engine.ml reset / step), host actions
//   ev_rollout_body        lockstep rollout on the device: every lane takes n_steps steps with
//                          the batch policy, auto-resetting finished episodes (gym VecEnv)
//   ev_observe_fields_body the observation's int32 fields
//
// Every __global__ kernel stays a shell in its protocol's translation unit (its name, its
// parameters, its occupancy attributes, its slab symbol) and calls the force-inlined body;
// the launchers below hold the layout and LDS guards once. Besides wave_sched.h's hooks the
// adapter gives
//   Slot, Obs, kObs            the lockstep slot {L, ep, last_ra, live}, the observation, its width
//   kSlab                      the lane keeps heap nodes / visibility rows in an LDS slab
//   kRollSched                 the rollout runs under wave-coherent dispatch (roll_fetch)
//   kEvLpw, kRollLpw           lanes per wave of the fused / rollout kernel when the kernel
//                              has no such parameter (64: every thread), 0 = the parameter
//   mem_at, node_mem, lane_bytes(P)
//   slab_attach / slab_load / slab_store   no-ops without a slab
//   slot_head(SL, hd)          the slot's head field, where it has one
//   head_at(L, P, M, hd)       the head as the hooks below take it (read and checked once)
//   reward_att, head, miner, acc, node_rews   the head's rewards and record fields, the
//                              summary's fixed-point scaling, the head's per-node reward row
//   observe, policy, write_obs, fields     the gym observation, the batch policy's action for
//                              the lane, the observation's encodings
//   trec_rows, fused_tail, roll_tail (host)   the kernels' trailing slab / lpw parameters
#pragma once
#include <hip/hip_runtime.h>

#include <tuple>

#include "kernels.h"
#include "summary.h"
#include "wave_sched.h"

namespace cpr {

constexpr bool kEvSched = CPR_EV_SCHED != 0;

inline unsigned grid_of(int64_t n) { return (unsigned)((n + kBlock - 1) / kBlock); }

// what a record or a step's info reports of the head
struct EvHead {
  double ra, rd, progress, time;
  int32_t height;
  int32_t rec_miner;  // cpr_episode_record.head_miner
  int32_t work;       // cpr_episode_record.head_work
};

// a workgroup's dynamic LDS (the kernel's slab symbol): kl heap nodes per lane, node-major,
// then the visibility rows of the newest vw vertices, then (tw > 0) Tailstorm's list-record
// window at byte tw_off (ev_slab_plan)
struct SlabView {
  bk::HNode* base;
  int32_t kl, vw, tw, tw_off;
};

// lpw lanes per wave run (lanes lpw..63 idle): fewer lanes per wave, more waves per SIMD to
// hide the dependent loads (rollout_lanes_per_wave, event_lanes_per_wave); the slab holds the
// used lanes' columns. LPW = 64: the kernel has no such parameter, every thread runs
struct LaneGeom {
  int32_t col, cols;  // the lane's column in the workgroup's slab, columns per workgroup
  int64_t id, total;  // the lane in the grid, lanes in the grid
  bool used;
};
template <int LPW>
__device__ __forceinline__ LaneGeom lane_geom(int32_t lpw) {
  LaneGeom g;
  if constexpr (LPW == 64) {
    g.col = (int32_t)threadIdx.x;
    g.cols = (int32_t)blockDim.x;
    g.id = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    g.total = (int64_t)gridDim.x * blockDim.x;
    g.used = true;
  } else {
    const int32_t wl = (int32_t)(threadIdx.x & 63u);
    const int32_t wpb = (int32_t)(blockDim.x >> 6);
    g.used = wl < lpw;
    g.col = (int32_t)(threadIdx.x >> 6) * lpw + (g.used ? wl : 0);
    g.cols = wpb * lpw;
    g.id = (int64_t)blockIdx.x * wpb * lpw + g.col;
    g.total = (int64_t)gridDim.x * wpb * lpw;
  }
  return g;
}

// what the three adapters share, and the hooks of a lane without a slab, a head field in its
// slot or kernel parameters of its own (an adapter hides what it has)
template <class LaneT, class ParT, class MemT>
struct EvAdapterBase {
  using Lane = LaneT;
  using Par = ParT;
  using Mem = MemT;
  template <class St>
  __device__ static void begin(Lane& L, const Par& P, const St& S, const Mem& M) {
    L.init(P, S, M);
  }
  __device__ static bool gym(const Par& P) { return P.mode == CPR_MODE_GYM; }
  __device__ static bool loop_attacker(const Par& P) { return P.net != 2; }
  __device__ __forceinline__ static void slab_attach(Mem&, const SlabView&, int32_t, int32_t) {}
  __device__ __forceinline__ static void slab_load(const Mem&, const Par&, const Lane&) {}
  __device__ __forceinline__ static void slab_store(const Mem&, const Lane&) {}
  template <class Slot>
  __device__ __forceinline__ static void slot_head(Slot&, int32_t) {}
  static int32_t trec_rows() { return 0; }
  static auto fused_tail(const EvSlab&, int32_t) { return std::make_tuple(); }
  static auto roll_tail(const EvSlab&, int32_t) { return std::make_tuple(); }
};

// -DCPR_EV_CLOCKS, a diagnostic build: shader-clock cycles of the wave per item class (the
// exec that follows the choice), of fetching (and finishing episodes) and of choosing, and
// the parts of the rollout's attack item; printed by lane 0 of a few workgroups
struct EvClocks {
#ifdef CPR_EV_CLOCKS
  uint64_t clk[WK_N + 2] = {};
  uint64_t sub[4] = {};  // the rollout's attack item: prepare, head/done, obs write, act
  uint32_t cnt[WK_N] = {};
  uint64_t tprev = clock64(), ta = 0;
  int32_t last = -1;
  __device__ void lap(uint64_t& to) {
    const uint64_t t = clock64();
    to += t - tprev;
    tprev = t;
  }
  __device__ void item() {
    uint64_t none = 0;
    lap(last >= 0 ? clk[last] : none);
  }
  __device__ void fetched() { lap(clk[WK_N]); }
  __device__ void chosen(int32_t k) {
    lap(clk[WK_N + 1]);
    last = k;
    ta = tprev;
    if (k >= 0) cnt[k] += 1;
  }
  __device__ void part(int32_t q) {
    const uint64_t t = clock64();
    sub[q] += t - ta;
    ta = t;
  }
  __device__ void print(bool parts) const {
    if (threadIdx.x != 0 || !(blockIdx.x == 0 || blockIdx.x == 77 || blockIdx.x == 200)) return;
    uint64_t tot = 0;
    for (int32_t q = 0; q < WK_N + 2; ++q) tot += clk[q];
    printf("EVCLK block %d total %llu fetch %llu choose %llu | clock %llu/%u dag %llu/%u "
           "tx %llu/%u rx %llu/%u on %llu/%u mv %llu/%u mdv %llu/%u attack %llu/%u "
           "pow0 %llu/%u\n",
           (int)blockIdx.x, (unsigned long long)tot, (unsigned long long)clk[WK_N],
           (unsigned long long)clk[WK_N + 1], (unsigned long long)clk[0], cnt[0],
           (unsigned long long)clk[1], cnt[1], (unsigned long long)clk[2], cnt[2],
           (unsigned long long)clk[3], cnt[3], (unsigned long long)clk[4], cnt[4],
           (unsigned long long)clk[5], cnt[5], (unsigned long long)clk[6], cnt[6],
           (unsigned long long)clk[7], cnt[7], (unsigned long long)clk[8], cnt[8]);
    if (parts)
      printf("EVCLK block %d attack: prepare %llu head %llu obs %llu act %llu\n",
             (int)blockIdx.x, (unsigned long long)sub[0], (unsigned long long)sub[1],
             (unsigned long long)sub[2], (unsigned long long)sub[3]);
  }
#else
  __device__ void item() {}
  __device__ void fetched() {}
  __device__ void chosen(int32_t) {}
  __device__ void part(int32_t) {}
  __device__ void print(bool) const {}
#endif
};

// one finished episode: summary, record, per-node row
template <class A, class Src, class St>
__device__ __forceinline__ void ev_finish(const typename A::Par& P, typename A::Lane& L,
                                 const typename A::Mem& M, const St& S, int64_t e, int32_t hd,
                                 Acc& acc, int32_t* hist, cpr_episode_record* recs,
                                 const NodeOut& no) {
  L.status |= Src::missed(S);
  const auto& hv = A::head_at(L, P, M, hd);
  A::acc(acc, P, L, M, hv, hist);
  if (recs) {
    const EvHead h = A::head(L, P, M, hv);
    cpr_episode_record r;
    r.reward_attacker = h.ra;
    r.reward_defender = h.rd;
    r.progress = h.progress;
    r.chain_time = h.time;
    r.sim_time = P.mode == CPR_MODE_GYM ? L.now : 0.0;
    r.n_steps = L.steps;
    r.n_activations = L.c_act;
    r.head_height = h.height;
    r.head_miner = h.rec_miner;
    r.status = L.status;
    r.head_work = h.work;
    recs[e] = r;
  }
  if (no.acts) {  // csv_runner.ml:74-79: sim.activations and (Dag.data head).rewards
    const auto rew = A::node_rews(L, P, M, hd, hv);
    for (int32_t j = 0; j < P.n; ++j) {
      no.acts[e * P.n + j] = M.nact[j];
      no.rews[e * P.n + j] = rew(j);
    }
    no.head_miner[e] = A::miner(hv);
  }
}

// the fused episode kernels: one lane = one episode at a time, grid-stride or work queue
template <class A, class Src>
__device__ __forceinline__ void ev_run_episodes_body(
    const typename A::Par& P, const Src& src, int64_t n_eps, uint8_t* mem, int64_t lane_bytes,
    cpr_episode_record* recs, cpr_summary* sum, const NodeOut& no, const SlabView& sv,
    int32_t lpw) {
  __shared__ int32_t hist[CPR_HIST_BINS];
  if (threadIdx.x < CPR_HIST_BINS) hist[threadIdx.x] = 0;
  __syncthreads();
  const LaneGeom g = lane_geom<A::kEvLpw>(lpw);
  typename A::Mem M = A::mem_at(mem + g.id * lane_bytes, P);
  if (no.mem) A::node_mem(M, no.mem + g.id * no.lane_bytes, P);
  // every episode starts with an empty heap and a fresh window (init): the slab needs no
  // load or store
  A::slab_attach(M, sv, g.col, g.cols);
  Acc acc = {};
  typename A::Lane L;
  if constexpr (kEvSched) {
    // wave-coherent dispatch (wave_sched.h): every iteration runs the work class most lanes
    // of the wave hold; episodes from a work queue, else grid-stride
    int64_t e = g.used ? g.id : n_eps;
    auto S = src.at(e < n_eps ? e : 0);
    EvCursor c;
    c.cls = -1;
    c.phase = PH_IDLE;
    if (e < n_eps) ev_begin<A>(L, P, S, M, c);
    EvClocks ck;
    for (;;) {
      ck.item();
      while (c.phase != PH_IDLE && c.cls < 0) {
        if (c.phase != PH_OVER) ev_fetch<A>(L, P, S, M, c);
        if (c.phase == PH_OVER) {
          ev_finish<A, Src>(P, L, M, S, e, c.hd, acc, hist, recs, no);
          e = ev_next_episode(P.next, e, g.total);
          if (e < n_eps) {
            S = src.at(e);
            ev_begin<A>(L, P, S, M, c);
          } else {
            c.phase = PH_IDLE;
          }
        }
      }
      ck.fetched();
      const int32_t k = ev_choose(c.cls);
      ck.chosen(k);
      if (k < 0) break;
      if (c.cls == k) ev_exec<A>(L, P, S, M, c);
    }
    ck.print(false);
  } else {
    for (int64_t e = g.used ? g.id : n_eps; e < n_eps; e += g.total) {
      const auto S = src.at(e);
      int32_t hd;
      if (P.mode == CPR_MODE_GYM) {
        L.gym_reset(P, S, M);
        bool done = L.dead != 0;
        hd = 0;
        while (!done) hd = L.gym_step(P, S, M, A::policy(L, P, M), &done);
      } else {
        hd = L.loop(P, S, M);
      }
      ev_finish<A, Src>(P, L, M, S, e, hd, acc, hist, recs, no);
    }
  }
  __syncthreads();
  block_flush(acc, hist, sum);
}

// engine.ml reward = Δ head.rewards[0]; episode ids of lane i in a rollout: i, i + n, ...
template <class A>
__device__ __forceinline__ void ev_slot_reset(const typename A::Par& P, uint64_t seed,
                                     const typename A::Mem& M, typename A::Slot& SL,
                                     uint64_t ep) {
  SL.ep = ep;
  SL.last_ra = 0.0;
  A::slot_head(SL, 0);
  SL.live = 1;
  SL.L.gym_reset(P, make_stream(seed, ep), M);
}

// LT: per-lane thresholds (lane_t) overwrite t_att in the kernel's by-value params; two
// instantiations, see k_reset in kernels.hip
template <class A, bool LT>
__device__ __forceinline__ void ev_reset_body(typename A::Par& P, uint64_t seed, uint8_t* mem,
                                              int64_t lane_bytes, typename A::Slot* slots,
                                              int64_t n, const uint8_t* mask,
                                              const uint64_t* eps, int unit, const double* tabs,
                                              int32_t tn, double* obs, const uint64_t* lane_t) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  if constexpr (LT) P.t_att = lane_t[i];  // the lane's own alpha (cpr_lane_env_set)
  const typename A::Mem M = A::mem_at(mem + i * lane_bytes, P);
  typename A::Slot SL = slots[i];
  if (mask == nullptr || mask[i]) ev_slot_reset<A>(P, seed, M, SL, eps ? eps[i] : (uint64_t)i);
  A::write_obs(P, A::observe(SL.L, P, M), unit, tabs, tn, obs + A::kObs * i);
  slots[i] = SL;
}

template <class A, bool LT>
__device__ __forceinline__ void ev_step_body(typename A::Par& P, uint64_t seed, uint8_t* mem,
                                             int64_t lane_bytes, typename A::Slot* slots,
                                             int64_t n, const int32_t* actions, int unit,
                                             const double* tabs, int32_t tn,
                                             const StepBuffers& out, const uint64_t* lane_t) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  if constexpr (LT) P.t_att = lane_t[i];  // the lane's own alpha (cpr_lane_env_set)
  const typename A::Mem M = A::mem_at(mem + i * lane_bytes, P);
  typename A::Slot SL = slots[i];
  bool done = false;
  const int32_t hd = SL.L.gym_step(P, make_stream(seed, SL.ep), M, actions[i], &done);
  A::slot_head(SL, hd);
  const auto& hv = A::head_at(SL.L, P, M, hd);
  const double ra = A::reward_att(SL.L, P, M, hv);
  out.reward[i] = ra - SL.last_ra;  // engine.ml:223
  out.done[i] = done ? 1 : 0;
  out.status[i] = SL.L.status;
  if (out.era) {
    const EvHead h = A::head(SL.L, P, M, hv);
    out.era[i] = h.ra;
    out.erd[i] = h.rd;
    out.eprog[i] = h.progress;
    out.ect[i] = h.time;
    out.est[i] = SL.L.now;
    out.esteps[i] = SL.L.steps;
    out.eacts[i] = SL.L.c_act;
    out.hh[i] = h.height;
    out.hm[i] = A::miner(hv);
  }
  SL.last_ra = ra;
  A::write_obs(P, A::observe(SL.L, P, M), unit, tabs, tn, out.obs + A::kObs * i);
  slots[i] = SL;
}

// n_steps lockstep steps per lane with the batch's on-device policy; finished episodes are
// summarised and the lane restarts with episode id ep + n (VecEnv auto-reset: the
// observation written at a done step is the new episode's first observation).
// summary.steps / .activations count every step / activation of the rollout; the other
// summary fields cover the episodes that finished in it.
template <class A>
__device__ __forceinline__ void ev_rollout_body(const typename A::Par& P, uint64_t seed,
                                                uint8_t* mem, int64_t lane_bytes,
                                                typename A::Slot* slots, int64_t n,
                                                int64_t n_steps, int unit, const double* tabs,
                                                int32_t tn, double* obs, double* reward,
                                                uint8_t* done_out, cpr_summary* sum,
                                                const SlabView& sv, int32_t lpw) {
  __shared__ int32_t hist[CPR_HIST_BINS];
  if (threadIdx.x < CPR_HIST_BINS) hist[threadIdx.x] = 0;
  __syncthreads();
  const LaneGeom g = lane_geom<A::kRollLpw>(lpw);
  const int64_t i = g.used ? g.id : n;
  Acc acc = {};
  int64_t steps_all = 0, acts_all = 0;
  if constexpr (kEvSched && A::kRollSched) {
    // wave-coherent dispatch (wave_sched.h roll_fetch): the plain loop below split into
    // items; every lane's own sequence of events, actions and outputs is the plain loop's
    typename A::Mem M = A::mem_at(mem + (i < n ? i : 0) * lane_bytes, P);
    // the lane's heap nodes 0 .. kl-1 move to the slab for this launch
    A::slab_attach(M, sv, g.col, g.cols);
    typename A::Slot SL;
    EvCursor c;
    c.cls = -1;
    c.phase = PH_IDLE;
    int64_t tk = 0;  // steps of this launch taken
    int32_t a0 = 0;  // activations of the current episode before this launch
    Stream S = make_stream(seed, 0);
    if (i < n) {
      SL = slots[i];
      A::slab_load(M, P, SL.L);
      if (!SL.live)
        ev_slot_reset<A>(P, seed, M, SL, (uint64_t)i);
      else
        a0 = SL.L.c_act;
      S = make_stream(seed, SL.ep);
      if (n_steps > 0) {
        A::act(SL.L, P, M);
        c.att = SL.L.priv;
        c.phase = PH_RUN;
      }
    }
    EvClocks ck;
    for (;;) {
      ck.item();
      if (c.phase != PH_IDLE && c.cls < 0) roll_fetch<A>(SL.L, M, c);
      ck.fetched();
      const int32_t kc = ev_choose(c.cls);
      ck.chosen(kc);
      if (kc < 0) break;
      if (c.cls != kc) continue;
      c.cls = -1;
      if (kc == WK_POW0) {
        A::run_pow0(SL.L, P, S, M, c.s);
        continue;
      }
      if (kc != WK_ATTACK) {
        SL.L.handle(P, S, M, c.ev, c.s);
        continue;
      }
      if (c.ev != kRollFail) SL.L.prepare(P, M, (c.ev >> 3) & 3u, c.s);
      ck.part(0);
      if (c.phase == PH_FRESH) {
        // the reset after a done step reached its first interaction: that step's observation
        c.phase = PH_RUN;
        if (obs)
          A::write_obs(P, A::observe(SL.L, P, M), unit, tabs, tn,
                       obs + A::kObs * ((tk - 1) * n + i));
      } else {
        const int32_t hd = A::head_gym(SL.L, P, M, c.att);
        const bool done = A::gym_done(SL.L, P, M, hd);
        ck.part(1);
        const auto& hv = A::head_at(SL.L, P, M, hd);
        const double ra = A::reward_att(SL.L, P, M, hv);
        const int64_t k = tk * n + i;
        if (reward) reward[k] = ra - SL.last_ra;
        if (done_out) done_out[k] = done ? 1 : 0;
        SL.last_ra = ra;
        ++tk;
        if (done) {
          A::acc(acc, P, SL.L, M, hv, hist);
          acts_all += SL.L.c_act - a0;
          a0 = 0;
          SL.ep += (uint64_t)n;  // ev_slot_reset, its events run as items
          SL.last_ra = 0.0;
          A::slot_head(SL, 0);
          SL.live = 1;
          S = make_stream(seed, SL.ep);
          SL.L.init(P, S, M);
          c.phase = PH_FRESH;
          continue;
        }
        if (obs) A::write_obs(P, A::observe(SL.L, P, M), unit, tabs, tn, obs + A::kObs * k);
      }
      ck.part(2);
      if (tk >= n_steps) {
        c.phase = PH_IDLE;  // at the decision point of the next launch's first step
        continue;
      }
      A::act(SL.L, P, M);
      c.att = SL.L.priv;
      ck.part(3);
    }
    if (i < n) {
      acts_all += SL.L.c_act - a0;
      steps_all = n_steps;
      A::slab_store(M, SL.L);
      slots[i] = SL;
    }
    ck.print(true);
  } else if (i < n) {
    typename A::Mem M = A::mem_at(mem + i * lane_bytes, P);
    typename A::Slot SL = slots[i];
    A::slab_attach(M, sv, g.col, g.cols);
    A::slab_load(M, P, SL.L);
    if (!SL.live) {
      ev_slot_reset<A>(P, seed, M, SL, (uint64_t)i);
      acts_all += SL.L.c_act;
    }
    for (int64_t t = 0; t < n_steps; ++t) {
      const int32_t a = A::policy(SL.L, P, M);
      const int32_t c0 = SL.L.c_act;
      bool done = false;
      const int32_t hd = SL.L.gym_step(P, make_stream(seed, SL.ep), M, a, &done);
      acts_all += SL.L.c_act - c0;
      ++steps_all;
      const auto& hv = A::head_at(SL.L, P, M, hd);
      const double ra = A::reward_att(SL.L, P, M, hv);
      const int64_t k = t * n + i;
      if (reward) reward[k] = ra - SL.last_ra;
      if (done_out) done_out[k] = done ? 1 : 0;
      SL.last_ra = ra;
      if (done) {
        A::acc(acc, P, SL.L, M, hv, hist);
        ev_slot_reset<A>(P, seed, M, SL, SL.ep + (uint64_t)n);
        acts_all += SL.L.c_act;
      }
      if (obs) A::write_obs(P, A::observe(SL.L, P, M), unit, tabs, tn, obs + A::kObs * k);
    }
    A::slab_store(M, SL.L);
    slots[i] = SL;
  }
  // rollout totals: all steps and activations (acc.steps/activations hold finished
  // episodes only, so replace them before the block reduction)
  acc.steps = steps_all;
  acc.activations = acts_all;
  __syncthreads();
  block_flush(acc, hist, sum);
}

template <class A>
__device__ __forceinline__ void ev_observe_fields_body(const typename A::Par& P, uint8_t* mem,
                                                       int64_t lane_bytes,
                                                       const typename A::Slot* slots, int64_t n,
                                                       int32_t* f) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const typename A::Mem M = A::mem_at(mem + i * lane_bytes, P);
  typename A::Lane L = slots[i].L;
  A::fields(A::observe(L, P, M), f + A::kObs * i);
}

// ---------------------------------------------------------------- launchers

// a fused episode kernel on the resident grid of `lanes` threads; lpw < 64 runs
// lanes * lpw / 64 episodes at a time in it
template <class A, class K, class Src>
hipError_t ev_launch_episodes(K kernel, const typename A::Par& P, const Src& src, int64_t n_eps,
                              uint8_t* mem, int64_t lane_bytes, int64_t lanes,
                              cpr_episode_record* recs, cpr_summary* sum, hipStream_t st,
                              const NodeOut& no) {
  CPR_LAYOUT_GUARD(lane_bytes, A::lane_bytes(P));
  const unsigned blocks = (unsigned)(lanes / kBlock);
  const int32_t lpw = A::kEvLpw ? A::kEvLpw : event_lanes_per_wave();
  EvSlab sl{0, 0, 0};
  if constexpr (A::kSlab) {
    sl = ev_slab_plan(blocks, (const void*)kernel, P.n, (kBlock / 64) * lpw, A::trec_rows());
    CPR_LDS_GUARD(kernel, sl.bytes);
  }
  std::apply(
      [&](auto... tail) {
        hipLaunchKernelGGL(kernel, dim3(blocks), dim3(kBlock), sl.bytes, st, P, src, n_eps, mem,
                           lane_bytes, recs, sum, no, tail...);
      },
      A::fused_tail(sl, lpw));
  return hipGetLastError();
}

template <class K>
int ev_blocks_per_cu(K kernel) {
  int blocks = 0;
  hipError_t e =
      hipOccupancyMaxActiveBlocksPerMultiprocessor(&blocks, (const void*)kernel, kBlock, 0);
  if (e != hipSuccess || blocks <= 0) blocks = 2;
  return blocks;
}

// one thread per lockstep lane: kernel(P, args...) over n lanes of lane_bytes each
template <class A, class K, class... Args>
hipError_t ev_launch_lanes(K kernel, int64_t lane_bytes, int64_t n, hipStream_t st,
                           const typename A::Par& P, Args... args) {
  CPR_LAYOUT_GUARD(lane_bytes, A::lane_bytes(P));
  hipLaunchKernelGGL(kernel, dim3(grid_of(n)), dim3(kBlock), 0, st, P, args...);
  return hipGetLastError();
}

template <class A, class K>
hipError_t ev_launch_rollout(K kernel, const typename A::Par& P, uint64_t seed, uint8_t* mem,
                             int64_t lane_bytes, void* slots, int64_t n, int64_t n_steps,
                             int unit, const double* tabs, int32_t tn, double* obs,
                             double* reward, uint8_t* done, cpr_summary* sum, hipStream_t st) {
  CPR_LAYOUT_GUARD(lane_bytes, A::lane_bytes(P));
  int32_t lpw = 64;
  unsigned blocks = grid_of(n);
  EvSlab sl{0, 0, 0};
  if constexpr (A::kSlab) {
    lpw = rollout_lanes_per_wave(n, (const void*)kernel);
    const int64_t per_block = (int64_t)(kBlock / 64) * lpw;
    blocks = (unsigned)((n + per_block - 1) / per_block);
    sl = ev_slab_plan(blocks, (const void*)kernel, P.n, (int32_t)per_block);
    CPR_LDS_GUARD(kernel, sl.bytes);
  }
  std::apply(
      [&](auto... tail) {
        hipLaunchKernelGGL(kernel, dim3(blocks), dim3(kBlock), sl.bytes, st, P, seed, mem,
                           lane_bytes, (typename A::Slot*)slots, n, n_steps, unit, tabs, tn, obs,
                           reward, done, sum, tail...);
      },
      A::roll_tail(sl, lpw));
  return hipGetLastError();
}

template <class A>
hipError_t ev_launch_cursor(const void* slots, int64_t n, const LaneCursor& c, hipStream_t st) {
  using Slot = typename A::Slot;
  hipLaunchKernelGGL(k_slot_cursor<Slot>, dim3(grid_of(n)), dim3(kBlock), 0, st,
                     (const Slot*)slots, n, c);
  return hipGetLastError();
}

}  // namespace cpr
