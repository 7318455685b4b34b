// k_run_episodes_fused: the two timed d = 2 summary kernels of kernels.hip for NA sweep
// points that share seed, first episode and episode count and differ only in alpha:
//   ARR = 0  k_run_episodes<GYM, SeedSource, POL, REC = 0, ARR = 0, TT = 1, LZ = 1> (gamma = 0)
//   ARR = 1  k_run_episodes<GYM, SeedSource, POL, REC = 0, ARR = 1, TT = 2, LZ = 2> (deferred
//            races: the gym's gamma = .5 network)
// One lane runs the NA points' state machines of one episode on one set of draws
// (nak_fused.h): the Philox block of an activation, the largest single cost of those
// kernels, is computed once instead of NA times; with lane groups (template parameter G) G
// adjacent lanes run NA points each of one episode and compute each block once between
// them, so once per NA * G points. Each point has its own summary, its own LDS
// accumulators, its own entry in the exact re-run's launch table and, with deferred races,
// its own list for the eager second pass; the results are those of NA separate launches,
// word for word.
#define CPR_UNIFORM_SEED 1
#include <hip/hip_runtime.h>

#include "../../include/cpr_hip.h"
#include "kernels.h"
#include "nak_fused.h"
#include "nak_rollout.h"
#include "summary.h"

#pragma clang fp contract(off)

namespace cpr {

template <int NA>
struct FuseArgs {
  FusePoint p[NA];
};

// deferred races: list entries per lane of a wave (one point: RQ_LANE, nakamoto_lane.h), so
// that a list is verified when about RQ_LANE entries per lane have gathered, as there
constexpr int32_t fused_rq_lane(int na) { return RQ_LANE + na - 1; }

// G: the lanes of a group (nak_fused.h "lane groups"): G adjacent lanes run one episode, lane g
// of a group the points g NA .. g NA + NA - 1 of the launch, and share each TAG_ACT block.
// G = 1: every lane its own episode and its own blocks.
// What a lane needs of its own points it reads from a copy of the points in LDS (G > 1):
// indexing the by-value argument with a per-lane index would put it into scratch memory, and
// selects over g kept every point's pointers in registers through the activation loop.
template <int POL, int NA, int ARR, int G>
__global__ __launch_bounds__(kBlock) void k_run_episodes_fused(NakParams P, SeedSource src,
                                                               int64_t n_eps,
                                                               FuseArgs<NA * G> A, int64_t* redo,
                                                               uint32_t* redo_n,
                                                               int64_t redo_cap) {
  static_assert(G == 1 || G == 2 || G == 4 || G == 8, "lanes per episode");
  P.arrive = ARR;  // as the one-point kernels: constants, so that the masks and loops fold
  P.d = 2;
  constexpr int32_t RQF = fused_rq_lane(NA);
  constexpr int NP = NA * G;  // the launch's points
  __shared__ int32_t hist[NP][CPR_HIST_BINS];
  __shared__ unsigned long long acc_w[NP][13];
  __shared__ uint4 rq[ARR ? RQF * kBlock : 1];
  __shared__ int32_t rflag[ARR ? kBlock : 1];
  __shared__ uint32_t rep[ARR ? 2 * kBlock : 1];
#pragma unroll
  for (int i = 0; i < NP; ++i) {
    if (threadIdx.x < 13) acc_w[i][threadIdx.x] = 0ull;
    if (threadIdx.x < CPR_HIST_BINS) hist[i][threadIdx.x] = 0;
  }
  const FusePoint* mine = nullptr;  // G > 1: the lane's own points, in LDS
  if constexpr (G > 1) {
    __shared__ FusePoint pts[NP];
#pragma unroll
    for (int i = 0; i < NP; ++i)
      if (threadIdx.x == i) pts[i] = A.p[i];
    mine = pts + (threadIdx.x & (G - 1)) * NA;
  }
  __syncthreads();
  const int64_t tid = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int64_t nthreads = (int64_t)gridDim.x * blockDim.x;
  const int32_t lane = (int32_t)(threadIdx.x % WAVE);
  const int32_t g = G > 1 ? lane & (G - 1) : 0;  // the lane in its group
  // summary only, ties by rule: no block times, no ring, no spill, no replay scratch
  LaneMem M;
  M.ring = nullptr;
  M.spill = nullptr;
  M.ring_stride = 0;
  M.spill_stride = 0;
  M.cap = P.cap;
  M.replay.nodes = nullptr;
  M.replay.masks = nullptr;
  M.times = false;
  M.d2 = true;
  // gym mode, one activation per step, and the launcher fuses only where cap >= max_steps + 2
  // (capi.hip fuse_kind): the private chain cannot reach its capacity
  M.cap_test = false;
  if constexpr (ARR != 0) {
    // each wave's race list, flags and episode words (as k_run_episodes, TT = 2)
    M.rq = rq + (threadIdx.x / WAVE) * (RQF * WAVE);
    M.rq_cap = RQF * WAVE;
    M.rflag = rflag + (threadIdx.x / WAVE) * WAVE;
    M.rep = rep + (threadIdx.x / WAVE) * (2 * WAVE);
    M.lane = lane;
    M.wave = WAVE;
    M.rflag[M.lane] = 0;
  }
  // of the lane's own point i (launch point g NA + i)
  auto own = [&](int i, auto field) {
    if constexpr (G > 1)
      return field(mine[i]);
    else
      return field(A.p[i]);
  };
  uint64_t t_att[NA];
#pragma unroll
  for (int i = 0; i < NA; ++i) t_att[i] = own(i, [](const FusePoint& p) { return p.t_att; });
  // tips packed into one word each (nakamoto_lane.h PTip): no block times here, and
  // lazy_clock_ok keeps every height and count below 2^16
  NakLanePacked L[NA];
  Words4 held{0u, 0u, 0u, 0u};  // G > 1: the block this lane computed for its group
  // a wave runs WAVE / G consecutive episodes, its grid nthreads / G
  for (int64_t e = tid / G; e < n_eps; e = nak_next_episode(P.next, e, nthreads / G, G)) {
    const Stream S = src.at(e);
#pragma unroll
    for (int i = 0; i < NA; ++i) L[i].init();
    fused_activate_w<NA, ARR>(L, P, S, M, t_att, group_block<G>(L, S, held, lane));
    // only max_steps ends the episode (lazy_clock_ok): the same trip count in every lane
    int64_t steps = 0;
    do {
      fused_step_pre<POL, NA, ARR>(L, P, S, M);
      fused_step_post<NA, ARR>(L, P, S, M, t_att, group_block<G>(L, S, held, lane));
      ++steps;
    } while (steps < P.max_steps);
    if constexpr (ARR != 0) fused_verify_races<NA>(L, P, S, M);
#pragma unroll
    for (int i = 0; i < NA; ++i) {
      const BRef hd = L[i].head(P, M);
      const uint32_t status = L[i].status;
      if (ARR && (status & ST_RACE_REDO)) {
        // a deferred race of this point went otherwise: the point's eager second pass runs
        // the episode again (list: count, then episode indices)
        int64_t* list = own(i, [](const FusePoint& p) { return p.list; });
        const uint32_t r = atomicAdd(reinterpret_cast<uint32_t*>(list), 1u);
        list[1 + r] = e;
      } else if (redo != nullptr && (status & kInexact) != 0u) {
        // this point's episode goes to the exact event engine under the point's own launch
        // (k_run_episodes); its siblings accumulate
        const uint32_t r = atomicAdd(redo_n, 1u);
        if ((int64_t)r < redo_cap)
          redo[r] = ((int64_t)own(i, [](const FusePoint& p) { return p.launch_id; }) << 40) |
                    (e << 8) | (int64_t)(status & 0xffu);
        else
          own(i, [](const FusePoint& p) { return p.ovf; })[e] =
              (uint8_t)(0x80u | (status & 0x7fu));
      } else {
        const double rel = hd.h != 0 ? (double)hd.ra / (double)hd.h : 0.0;
        const int pt = g * NA + i;
        LdsAcc acc{acc_w[pt]};
        acc.episode((int64_t)hd.ra << 20, (int64_t)(hd.h - hd.ra) << 20, (int64_t)hd.h << 20, rel,
                    hd.h, steps, L[0].k, status, hist[pt]);
      }
    }
  }
  __syncthreads();
#pragma unroll
  for (int i = 0; i < NP; ++i) {
    const LdsAcc acc{acc_w[i]};
    acc.flush(hist[i], A.p[i].sum);
  }
}

using FusedFn = const void*;

template <int POL, int NA, int ARR, int G>
static hipError_t launch_fused(const NakParams& P, const SeedSource& src, int64_t n_eps,
                               const FusePoint* pts, unsigned blocks, int64_t* redo,
                               uint32_t* redo_n, int64_t redo_cap, hipStream_t st, FusedFn* fn) {
  if (fn) {
    *fn = (const void*)k_run_episodes_fused<POL, NA, ARR, G>;
    return hipSuccess;
  }
  FuseArgs<NA * G> A;
  for (int i = 0; i < NA * G; ++i) A.p[i] = pts[i];
  hipLaunchKernelGGL((k_run_episodes_fused<POL, NA, ARR, G>), dim3(blocks), dim3(kBlock), 0, st,
                     P, src, n_eps, A, redo, redo_n, redo_cap);
  return hipGetLastError();
}

// na points per lane, g lanes per episode: g = 1 with na in 2 .. MAX; g a power of two up to
// the kind's largest built group, full lanes only (na = MAX)
template <int POL, int ARR>
static hipError_t launch_fused_na(int na, int g, const NakParams& P, const SeedSource& src,
                                  int64_t n_eps, const FusePoint* pts, unsigned blocks,
                                  int64_t* redo, uint32_t* redo_n, int64_t redo_cap,
                                  hipStream_t st, FusedFn* fn) {
  constexpr int MAX = ARR ? CPR_NAK_FUSE_MAX_ARR : CPR_NAK_FUSE_MAX;
  constexpr int GMAX = ARR ? CPR_NAK_FUSE_LANES_ARR : CPR_NAK_FUSE_LANES;
  if (g > 1) {
    if (na != MAX) return hipErrorInvalidValue;
    switch (g) {
#define CPR_FUSED_LANES(G)                                                                   \
  case G:                                                                                    \
    if constexpr (G <= GMAX)                                                                 \
      return launch_fused<POL, MAX, ARR, G>(P, src, n_eps, pts, blocks, redo, redo_n,        \
                                            redo_cap, st, fn);                               \
    return hipErrorInvalidValue;
      CPR_FUSED_LANES(2)
      CPR_FUSED_LANES(4)
      CPR_FUSED_LANES(8)
#undef CPR_FUSED_LANES
      default: return hipErrorInvalidValue;
    }
  }
  switch (na) {
#define CPR_FUSED_CASE(N)                                                                    \
  case N:                                                                                    \
    if constexpr (N <= MAX)                                                                  \
      return launch_fused<POL, N, ARR, 1>(P, src, n_eps, pts, blocks, redo, redo_n,          \
                                          redo_cap, st, fn);                                 \
    return hipErrorInvalidValue;
    CPR_FUSED_CASE(2)
    CPR_FUSED_CASE(3)
    CPR_FUSED_CASE(4)
    CPR_FUSED_CASE(5)
#undef CPR_FUSED_CASE
    default: return hipErrorInvalidValue;
  }
}

// fn: null to launch; else only the instantiation's address is returned (occupancy query)
static hipError_t fused_dispatch(int na, int g, const NakParams& P, const SeedSource& src,
                                 int64_t n_eps, const FusePoint* pts, unsigned blocks,
                                 int64_t* redo, uint32_t* redo_n, int64_t redo_cap,
                                 hipStream_t st, FusedFn* fn) {
#define CPR_FUSED_POL(POL)                                                                    \
  case POL:                                                                                   \
    return P.arrive ? launch_fused_na<POL, 1>(na, g, P, src, n_eps, pts, blocks, redo,        \
                                              redo_n, redo_cap, st, fn)                       \
                    : launch_fused_na<POL, 0>(na, g, P, src, n_eps, pts, blocks, redo,        \
                                              redo_n, redo_cap, st, fn);
  switch (P.policy) {
    CPR_FUSED_POL(P_HONEST)
    CPR_FUSED_POL(P_SIMPLE)
    CPR_FUSED_POL(P_ES2014)
    CPR_FUSED_POL(P_SM1)
#undef CPR_FUSED_POL
    default: return hipErrorInvalidValue;
  }
}

hipError_t launch_run_episodes_fused(const NakParams& P0, uint64_t seed, uint64_t first,
                                     int64_t n_eps, const FusePoint* pts, int na, int g,
                                     int64_t lanes, int64_t* redo, uint32_t* redo_n,
                                     int64_t redo_cap, hipStream_t st) {
  NakParams P = P0;
  P.u_lazy = lazy_threshold(P0);
  if (P.arrive) {
    // deferred races: every point's list (1 + n_eps words) receives the episodes for its
    // eager second pass (launch_run_episodes_second), its count first
    for (int i = 0; i < na * g; ++i) {
      const hipError_t er = hipMemsetAsync(pts[i].list, 0, sizeof(int64_t), st);
      if (er != hipSuccess) return er;
    }
  }
  return fused_dispatch(na, g, P, SeedSource{seed, first}, n_eps, pts,
                        (unsigned)(lanes / kBlock), redo, redo_n, redo_cap, st, nullptr);
}

int run_episodes_fused_blocks_per_cu(const NakParams& P, int na, int g) {
  FusedFn fn = nullptr;
  int blocks = 0;
  if (fused_dispatch(na, g, P, SeedSource{0, 0}, 0, nullptr, 0, nullptr, nullptr, 0, nullptr,
                     &fn) != hipSuccess ||
      hipOccupancyMaxActiveBlocksPerMultiprocessor(&blocks, fn, kBlock, 0) != hipSuccess ||
      blocks <= 0)
    blocks = 1;
  return blocks;
}

}  // namespace cpr
