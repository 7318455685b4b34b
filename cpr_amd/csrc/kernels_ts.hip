// Tailstorm kernels for gfx950: one lane = one episode / gym env of the tailstorm_ssz
// attack space, driven by the exact per-lane event engine of ts_lane.h. This unit holds what
// is Tailstorm's own: the adapter (TsAdapter: slot, head rewards, observation encodings,
// slab hooks with the list-record window), the policy decode kernel, and the kernel shells
// (k_ts_run_episodes, k_ts_reset / k_ts_step, k_ts_rollout) with their names, occupancy and
// slab symbol. The kernel bodies and the launchers are ev_kernels.h's.
#include <hip/hip_runtime.h>

// occupancy of this TU's event-engine kernels (kernels.h CPR_EV_OCC): 2 waves/SIMD measured
// +35 % over the unconstrained build on the configs[3] exp-clique probe under wave-coherent
// dispatch (profiles/r03f_event_occupancy_ab.log); build_variants.py overrides it with -D
#ifndef CPR_EV_WAVES
#define CPR_EV_WAVES 2
#endif

#include <algorithm>
#include <cstdlib>

#include "../../include/cpr_hip.h"
#include "ev_kernels.h"
#include "ts_lane.h"

#pragma clang fp contract(off)

namespace cpr {

struct TsSlot {
  ts::TsLane L;
  uint64_t ep;
  double last_ra;
  int32_t live;
};

// ev_kernels.h / wave_sched.h adapter: gym episodes (engine.ml reset / step with the
// on-device policy) and Simulator.loop tasks of ts_lane.h
struct TsAdapter : EvAdapterBase<ts::TsLane, ts::TsParams, ts::TsMem> {
  using Slot = TsSlot;
  using Obs = ts::TsObs;
  static constexpr int kObs = 10;
  static constexpr bool kSlab = true, kRollSched = true;
  static constexpr int kEvLpw = 0, kRollLpw = 0;

  __device__ static bool pow0(uint32_t ev) {
    return (ev & 7u) == ts::EV_DAG && (ev >> 5) == 0u && ((ev >> 3) & 3u) == ts::KD_POW;
  }
  template <class St>
  __device__ __forceinline__ static void run_pow0(Lane& L, const Par& P, const St& S,
                                                  const Mem& M, int32_t) {
    const int32_t v = L.append_vote(P, S, M, 0, L.payload_parent(P, M, 0, L.priv));
    L.push_now(P, M, bk::mkev(ts::EV_MV, 0, ts::KD_POW), v);
  }
  __device__ __forceinline__ static Obs observe(Lane& L, const Par& P, const Mem& M) {
    return L.observe(P, M);
  }
  __device__ __forceinline__ static int32_t policy(Lane& L, const Par& P, const Mem& M) {
    return ts::ts_policy_p(P, L.observe(P, M));
  }
  __device__ static void act(Lane& L, const Par& P, const Mem& M) {
    L.apply(P, M, policy(L, P, M));
    ++L.steps;
  }
  __device__ static int32_t head_gym(Lane& L, const Par& P, const Mem& M, int32_t att) {
    return L.dead ? 0 : L.head(P, M, att);
  }
  __device__ static int32_t head_loop(Lane& L, const Par& P, const Mem& M) {
    return L.dead ? 0 : L.head(P, M, P.net == 2 ? M.tips[0] : L.priv);
  }
  __device__ static bool gym_done(Lane& L, const Par& P, const Mem& M, int32_t hd) {
    const double progress = (double)(L.X(P, M, hd).height * P.k);
    return L.dead || !(L.steps < P.max_steps && progress < P.max_progress && L.now < P.max_time);
  }

  __host__ __device__ static int64_t lane_bytes(const Par& P) { return ts::ts_lane_bytes(P); }
  __device__ __forceinline__ static Mem mem_at(uint8_t* base, const Par& P) {
    return ts::ts_mem_at(base, P);
  }
  __device__ __forceinline__ static void node_mem(Mem& M, uint8_t* base, const Par&) {
    M.nact = (int64_t*)base;
  }
  __device__ __forceinline__ static void slab_attach(Mem& M, const SlabView& s, int32_t col,
                                                     int32_t cols) {
    ts::ts_heap_slab(M, s.base, col, cols, s.kl);
    ts::ts_vis_window(M, (uint8_t*)(s.base + (size_t)s.kl * cols), col, s.vw);
    if (s.tw > 0) ts::ts_trec_window(M, (ts::TRec*)((uint8_t*)s.base + s.tw_off), col, s.tw);
  }
  __device__ __forceinline__ static void slab_load(const Mem& M, const Par& P, const Lane& L) {
    ts::ts_heap_load(M, L.hused);
    ts::ts_vis_load(M, P, L.newest);
  }
  __device__ __forceinline__ static void slab_store(const Mem& M, const Lane& L) {
    ts::ts_heap_store(M, L.hused);
  }

  // head rewards: engine.ml:215-219 folds head.rewards left to right
  __device__ __forceinline__ static void head_rewards(const Par& P, Lane& L, const Mem& M,
                                                      int32_t hd, double* ra, double* rd) {
    const ts::TVtx& h = L.X(P, M, hd);
    *ra = 0.0;
    *rd = 0.0;
    if (h.qslot < 0) return;
    const double* rw = L.R(P, M, h.qslot);
    *ra = rw[0];
    double s = 0.0;
    for (int32_t j = 1; j < P.n; ++j) s += rw[j];
    *rd = s;
  }
  // the hooks read the head vertex themselves (X, R)
  __device__ __forceinline__ static int32_t head_at(Lane&, const Par&, const Mem&, int32_t hd) {
    return hd;
  }
  __device__ __forceinline__ static double reward_att(Lane& L, const Par& P, const Mem& M,
                                                      int32_t hd) {
    double ra, rd;
    head_rewards(P, L, M, hd, &ra, &rd);
    return ra;
  }
  __device__ __forceinline__ static EvHead head(Lane& L, const Par& P, const Mem& M, int32_t hd) {
    EvHead r;
    head_rewards(P, L, M, hd, &r.ra, &r.rd);
    const ts::TVtx& h = L.X(P, M, hd);
    r.progress = (double)(h.height * P.k);
    r.time = h.time;
    r.height = h.height;
    r.rec_miner = -1;
    r.work = 0;
    return r;
  }
  // summaries have no miner (tailstorm.ml info: kind, height)
  __device__ __forceinline__ static int32_t miner(int32_t) { return -1; }
  __device__ __forceinline__ static void acc(Acc& acc, const Par& P, Lane& L, const Mem& M,
                                             int32_t hd, int32_t* hist) {
    double ra, rd;
    head_rewards(P, L, M, hd, &ra, &rd);
    const int32_t h = L.X(P, M, hd).height;
    const double rel = (ra + rd) != 0.0 ? ra / (ra + rd) : 0.0;
    acc_episode(acc, (int64_t)__builtin_rint(ra * 1048576.0),
                (int64_t)__builtin_rint(rd * 1048576.0), (int64_t)h * P.k << 20, rel,
                (int64_t)h * P.k, L.steps, L.c_act, L.status, hist);
  }
  __device__ __forceinline__ static auto node_rews(Lane& L, const Par& P, const Mem& M,
                                                   int32_t hd, int32_t) {
    const ts::TVtx& h = L.X(P, M, hd);
    const double* hr = h.qslot < 0 ? nullptr : L.R(P, M, h.qslot);
    return [hr](int32_t j) { return hr ? hr[j] : 0.0; };
  }

  __device__ __forceinline__ static void fields(const Obs& o, int32_t* g) {
    const int32_t v[10] = {o.public_blocks,           o.private_blocks,
                           o.diff_blocks,             o.public_votes,
                           o.private_votes_inclusive, o.private_votes_exclusive,
                           o.public_depth,            o.private_depth_inclusive,
                           o.private_depth_exclusive, o.event};
    for (int j = 0; j < 10; ++j) g[j] = v[j];
  }
  // tailstorm_ssz.ml:41-55 normalizers; tabs as in BkAdapter::write_obs
  __device__ __forceinline__ static void write_obs(const Par& P, const Obs& o, int unit,
                                                   const double* tabs, int32_t tn, double* out) {
    const double pi = 3.141592653589793;
    int32_t v[10];
    fields(o, v);
    if (!unit) {
      for (int i = 0; i < 10; ++i) out[i] = (double)v[i];
      return;
    }
    for (int i = 0; i < 9; ++i) {
      const int32_t x = v[i];
      if (i == 2)
        out[i] = (x > -tn && x < tn) ? tabs[tn + x + tn] : 0.5 + (1.0 / pi * atan((double)x / 1.0));
      else if (i < 2)
        out[i] = x < tn ? tabs[x] : 2.0 / pi * atan((double)x / 1.0);
      else
        out[i] = x < tn ? tabs[3 * tn + x] : 2.0 / pi * atan((double)x / (double)P.k);
    }
    out[9] = (double)v[9] / 2.0;
  }

  // the fused kernel's list-record window rows (TsMem.tl, ev_slab_plan): 8 (configs[3] +2.6 %
  // in kernel, the exp-delay variant +0.5 %, profiles/r6q_ts_trec_window_ab.log; 16 rows leave
  // no heap slab and lose); CPR_TS_TWIN overrides (0 = none) for A/B runs
  static int32_t trec_rows() {
    if (const char* v = getenv("CPR_TS_TWIN")) return std::max(0, std::min(64, atoi(v)));
    return 8;
  }
  // the kernels' parameters after the shared ones
  static auto fused_tail(const EvSlab& sl, int32_t lpw) {
    return std::make_tuple(sl.kl, sl.vw, lpw, sl.tw, (int32_t)sl.tw_off);
  }
  static auto roll_tail(const EvSlab& sl, int32_t lpw) {
    return std::make_tuple(sl.kl, sl.vw, lpw);
  }
};

// the heap slab of a workgroup (dynamic LDS): kl nodes per lane, node-major
extern __shared__ __attribute__((aligned(16))) bk::HNode ts_slab[];

template <class Src>
__global__ __launch_bounds__(kBlock) CPR_EV_OCC void k_ts_run_episodes(
    ts::TsParams P, Src src, int64_t n_eps, uint8_t* mem, int64_t lane_bytes,
    cpr_episode_record* recs, cpr_summary* sum, NodeOut no, int32_t kl, int32_t vw, int32_t lpw,
    int32_t tw, int32_t tw_off) {
  ev_run_episodes_body<TsAdapter, Src>(P, src, n_eps, mem, lane_bytes, recs, sum, no,
                                       SlabView{ts_slab, kl, vw, tw, tw_off}, lpw);
}

template <bool LT>
__global__ __launch_bounds__(kBlock) void k_ts_reset(
    ts::TsParams P, uint64_t seed, uint8_t* mem, int64_t lane_bytes, TsSlot* slots, int64_t n,
    const uint8_t* mask, const uint64_t* eps, int unit, const double* tabs, int32_t tn, double* obs,
    const uint64_t* lane_t) {
  ev_reset_body<TsAdapter, LT>(P, seed, mem, lane_bytes, slots, n, mask, eps, unit, tabs, tn,
                               obs, lane_t);
}

template <bool LT>
__global__ __launch_bounds__(kBlock) void k_ts_step(
    ts::TsParams P, uint64_t seed, uint8_t* mem, int64_t lane_bytes, TsSlot* slots, int64_t n,
    const int32_t* actions, int unit, const double* tabs, int32_t tn, StepBuffers out,
    const uint64_t* lane_t) {
  ev_step_body<TsAdapter, LT>(P, seed, mem, lane_bytes, slots, n, actions, unit, tabs, tn, out,
                              lane_t);
}

__global__ __launch_bounds__(kBlock) CPR_EV_OCC void k_ts_rollout(
    ts::TsParams P, uint64_t seed, uint8_t* mem, int64_t lane_bytes, TsSlot* slots, int64_t n,
    int64_t n_steps, int unit, const double* tabs, int32_t tn, double* obs, double* reward,
    uint8_t* done_out, cpr_summary* sum, int32_t kl, int32_t vw, int32_t lpw) {
  ev_rollout_body<TsAdapter>(P, seed, mem, lane_bytes, slots, n, n_steps, unit, tabs, tn, obs,
                             reward, done_out, sum, SlabView{ts_slab, kl, vw, 0, 0}, lpw);
}

__global__ void k_ts_observe_fields(
    ts::TsParams P, uint8_t* mem, int64_t lane_bytes, const TsSlot* slots, int64_t n, int32_t* f) {
  ev_observe_fields_body<TsAdapter>(P, mem, lane_bytes, slots, n, f);
}

// engine.ml:258-261 on encoded observations (ssz_tools.ml:42-58 of_float)
__global__ void k_ts_policy(int32_t policy, int32_t k, int unit, const double* obs, int64_t n,
                            const uint8_t* table, int32_t dim, int32_t* actions) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const double* x = obs + 10 * i;
  const double pi = 3.141592653589793;
  int32_t v[10];
  for (int j = 0; j < 10; ++j) {
    if (j == 9) {
      v[j] = unit ? (int32_t)floor(x[j] * 2.0) : (int32_t)x[j];
    } else if (!unit) {
      v[j] = (int32_t)x[j];
    } else {
      const double scale = j >= 3 ? (double)k : 1.0;
      v[j] = j == 2 ? (int32_t)__builtin_round(tan(pi * (x[j] - 0.5)) * scale)
                    : (int32_t)__builtin_round(tan(pi / 2.0 * x[j]) * scale);
    }
  }
  const ts::TsObs o{v[0], v[1], v[2], v[3], v[4], v[5], v[6], v[7], v[8], v[9]};
  actions[i] = ts::ts_policy_t(policy, k, o, table, dim);
}

// ---------------------------------------------------------------- launchers

hipError_t launch_ts_run_episodes(const ts::TsParams& P, uint64_t seed, uint64_t first,
                                  int64_t n_eps, uint8_t* mem, int64_t lane_bytes, int64_t lanes,
                                  cpr_episode_record* recs, cpr_summary* sum, hipStream_t st,
                                  const NodeOut& no) {
  return ev_launch_episodes<TsAdapter>(k_ts_run_episodes<SeedSource>, P, SeedSource{seed, first},
                                       n_eps, mem, lane_bytes, lanes, recs, sum, st, no);
}

hipError_t launch_ts_replay_episodes(const ts::TsParams& P, const TraceSource& src, int64_t n_eps,
                                 uint8_t* mem, int64_t lane_bytes, int64_t lanes,
                                 cpr_episode_record* recs, cpr_summary* sum, hipStream_t st,
                                  const NodeOut& no) {
  return ev_launch_episodes<TsAdapter>(k_ts_run_episodes<TraceSource>, P, src, n_eps, mem,
                                       lane_bytes, lanes, recs, sum, st, no);
}

hipError_t launch_ts_reset(const ts::TsParams& P, uint64_t seed, uint8_t* mem, int64_t lane_bytes,
                           void* slots, int64_t n, const uint8_t* mask, const uint64_t* eps,
                           int unit, const double* tabs, int32_t tn, double* obs,
                           hipStream_t st, const uint64_t* lane_t) {
  return ev_launch_lanes<TsAdapter>(lane_t ? k_ts_reset<true> : k_ts_reset<false>, lane_bytes, n,
                                    st, P, seed, mem, lane_bytes, (TsSlot*)slots, n, mask, eps,
                                    unit, tabs, tn, obs, lane_t);
}

hipError_t launch_ts_step(const ts::TsParams& P, uint64_t seed, uint8_t* mem, int64_t lane_bytes,
                          void* slots, int64_t n, const int32_t* actions, int unit,
                          const double* tabs, int32_t tn, const StepBuffers& b, hipStream_t st,
                          const uint64_t* lane_t) {
  return ev_launch_lanes<TsAdapter>(lane_t ? k_ts_step<true> : k_ts_step<false>, lane_bytes, n, st,
                                    P, seed, mem, lane_bytes, (TsSlot*)slots, n, actions, unit,
                                    tabs, tn, b, lane_t);
}

hipError_t launch_ts_rollout(const ts::TsParams& P, uint64_t seed, uint8_t* mem,
                             int64_t lane_bytes, void* slots, int64_t n, int64_t n_steps,
                             int unit, const double* tabs, int32_t tn, double* obs,
                             double* reward, uint8_t* done, cpr_summary* sum, hipStream_t st) {
  return ev_launch_rollout<TsAdapter>(k_ts_rollout, P, seed, mem, lane_bytes, slots, n, n_steps,
                                      unit, tabs, tn, obs, reward, done, sum, st);
}

hipError_t launch_ts_observe_fields(const ts::TsParams& P, uint8_t* mem, int64_t lane_bytes,
                                    const void* slots, int64_t n, int32_t* f, hipStream_t st) {
  return ev_launch_lanes<TsAdapter>(k_ts_observe_fields, lane_bytes, n, st, P, mem, lane_bytes,
                                    (const TsSlot*)slots, n, f);
}

hipError_t launch_ts_cursor(const void* slots, int64_t n, const LaneCursor& c, hipStream_t st) {
  return ev_launch_cursor<TsAdapter>(slots, n, c, st);
}

hipError_t launch_ts_policy(int32_t policy, int32_t k, int unit, const double* obs, int64_t n,
                            const uint8_t* table, int32_t dim, int32_t* actions,
                            hipStream_t st) {
  hipLaunchKernelGGL(k_ts_policy, dim3(grid_of(n)), dim3(kBlock), 0, st, policy, k, unit, obs, n,
                     table, dim, actions);
  return hipGetLastError();
}

size_t ts_slot_bytes() { return sizeof(TsSlot); }

int ts_blocks_per_cu() { return ev_blocks_per_cu(k_ts_run_episodes<SeedSource>); }

}  // namespace cpr
