// NA sweep points in one lane (k_run_episodes_fused, kernels_nak_fused.hip): gym episodes of
// the two timed d = 2 summary kernels (no block times, lazy clock, ties by rule; gamma = 0:
// ARR = 0, LZ = 1, TT = 1; gamma = .5: ARR = 1, LZ = 2, deferred races TT = 2) that share
// seed, episode and activation count, and so every draw of the keyed stream. The TAG_ACT
// block of an activation depends on (seed, episode, activation count) alone; a point's alpha
// enters only afterwards, as the threshold that names the miner. So the block, the clock
// uniform, the lazy clock's skip test, the clock bound of the deferred races (lz_term, esum)
// and, in the rare exact branch, the clock sums are computed once per activation, and each
// point keeps only its own NakLane. The loops over the points have a compile-time trip count
// and are unrolled in full: the states stay in registers and no array of lanes is indexed
// dynamically.
// Lane groups (below): the lanes of a wave that run further points of the same episode compute
// one block per G activations each and pass them round in registers.
// The functions are generic over the lane type LN: NakLane, or NakLanePacked as the kernel
// runs them (tests/native_tips runs the two side by side).
// Compiles for the host like nakamoto_lane.h (tests/native_fused and tests/native_lane_groups
// run it beside single lanes).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "nakamoto_lane.h"

#pragma clang fp contract(off)

// the largest group (points per lane) an instantiation is built for: sizes 2 .. this
#ifndef CPR_NAK_FUSE_MAX
#define CPR_NAK_FUSE_MAX 5
#endif
// the same for the deferred-race kernel (gamma = .5), whose points hold more state: with
// whole tips 121 VGPRs at two points (4 waves/SIMD), 149 / 178 / 206 at three to five (3 / 2 /
// 2 waves), which measured no faster than two (DESIGN.md "Sweep points in one lane"); with
// packed tips 109 at two and 130 at three, still 3 waves (DESIGN.md "Packed tips")
#ifndef CPR_NAK_FUSE_MAX_ARR
#define CPR_NAK_FUSE_MAX_ARR 2
#endif
// the largest lane group (lanes that share an episode and its TAG_ACT blocks, below) a kernel
// with full lanes is built for, per kind: powers of two 2 .. this; 1: none
#ifndef CPR_NAK_FUSE_LANES
#define CPR_NAK_FUSE_LANES 2
#endif
#ifndef CPR_NAK_FUSE_LANES_ARR
#define CPR_NAK_FUSE_LANES_ARR 4
#endif

namespace cpr {

// What the points of a lane share lives in the first lane: k, tinf, and with the deferred
// races esum and qn (the stream's and the wave's: the same in every point).

// NakLane::lazy_overlap_check for the points of one lane: the same comparisons on the same
// sums, the sums (tp, tn: functions of the stream and the activation count) taken once.
// d = 2; ARR = 0 (gamma = 0): the previous window's only message is its defender block
// (always inlined: a call would take the lanes' address and put them in scratch memory)
template <int NA, int ARR, class St, class LN>
__host__ __device__ inline CPR_AI void fused_lazy_check(LN (&L)[NA], const NakParams& P,
                                                        const St& S, uint64_t u) {
  bool wb[NA], wr[NA], any = false;
#pragma unroll
  for (int i = 0; i < NA; ++i) {
    wb[i] = L[i].w_hasb != 0;
    wr[i] = ARR != 0 && L[i].rhi >= L[i].rlo;  // the previous window's release
    any |= wb[i] | wr[i];
  }
  if (L[0].tinf) {
#pragma unroll
    for (int i = 0; i < NA; ++i) L[i].status |= (wb[i] | wr[i]) ? (uint32_t)ST_OVERLAP : 0u;
    return;
  }
  if (u == 0ull) {  // this activation's delay is +inf
#pragma unroll
    for (int i = 0; i < NA; ++i) L[i].tinf = 1;
    return;
  }
  if (!any) return;
  const int32_t k = L[0].k;
  double tp = 0.0;
  for (int32_t j = 0; j < k; ++j) tp = tp + S.clock((uint32_t)j, P.ev);
  const double tn = tp + S.clock((uint32_t)k, P.ev);
#pragma unroll
  for (int i = 0; i < NA; ++i) {
    if (!(wb[i] | wr[i])) continue;
    double bound = wb[i] ? tp + P.delta : -__builtin_inf();
    if (wr[i]) {
      const double ub = tp + (P.dmax - 0.0);
      bound = ub > bound ? ub : bound;
    }
    if (tn <= bound) {
      if (tn <= L[i].window_last_arrival_at(P, S, tp)) L[i].status |= ST_OVERLAP;
    }
  }
}

// the next activation of every point from its counter block w: one block, NA miners
template <int NA, int ARR, class St, class LN>
__host__ __device__ inline CPR_AI void fused_activate_w(LN (&L)[NA], const NakParams& P,
                                                        const St& S, const LaneMem& M,
                                                        const uint64_t (&t_att)[NA],
                                                        const Words4& w) {
  const uint64_t u = ((uint64_t)(w.w2 >> 5) << 26) | (uint64_t)(w.w3 >> 6);  // Stream::act_u
  const uint32_t uh = (uint32_t)(u >> 26);
  // NakLane::activate's skip test
  if ((uh - 1u) >= (lazy_hi(P.u_lazy) - 1u) || L[0].tinf) fused_lazy_check<NA, ARR>(L, P, S, u);
  if constexpr (ARR != 0) L[0].esum += LN::lz_term(u);
#pragma unroll
  for (int i = 0; i < NA; ++i) {
    typename LN::Draw dr;
    dr.dt = 0.0;
    dr.u = u;
    dr.miner = miner_from_words(w.w0, w.w1, t_att[i], 2);
    L[i].template activate<St, ARR ? 2 : 1, false>(P, S, M, dr);
  }
}

template <int NA, int ARR, class St, class LN>
__host__ __device__ inline CPR_AI void fused_activate(LN (&L)[NA], const NakParams& P,
                                                      const St& S, const LaneMem& M,
                                                      const uint64_t (&t_att)[NA]) {
  fused_activate_w<NA, ARR>(L, P, S, M, t_att, S.block((uint32_t)L[0].k, TAG_ACT));
}

// reset of every point: up to the attacker's first interaction
template <int NA, int ARR, class St, class LN>
__host__ __device__ inline CPR_AI void fused_reset(LN (&L)[NA], const NakParams& P,
                                                   const St& S, const LaneMem& M,
                                                   const uint64_t (&t_att)[NA]) {
#pragma unroll
  for (int i = 0; i < NA; ++i) L[i].init();
  fused_activate<NA, ARR>(L, P, S, M, t_att);
}

// ---- deferred races of NA points (ARR = 1): one list per wave, as for one point; an entry
// carries its point in y (bit 0: the clock is +inf; bits 1..: the point), and the wave's
// flag word of a lane holds two bits per point (races_check<.., NP>)

// enqueue_race for every point, in point order
template <int NA, class LN>
__host__ __device__ inline CPR_AI void fused_enqueue_races(LN (&L)[NA], const LaneMem& M) {
  int32_t qn = L[0].qn;
#pragma unroll
  for (int i = 0; i < NA; ++i) {
    const bool race = L[i].rw != 0u;
    const uint64_t bal = wave_ballot(race);
    if (race) {
      uint4 e;
      e.x = L[0].esum;
      e.y = (uint32_t)L[0].tinf | ((uint32_t)i << 1);
      e.z = (uint32_t)L[0].k;
      e.w = L[i].rw | ((uint32_t)M.lane << 26);
      M.rq[qn + lanes_below(bal)] = e;
    }
    qn += __builtin_popcountll(bal);
    L[i].rw = 0u;
  }
  L[0].qn = qn;
}

// the list must be verified before the next iteration's NA races per lane could overflow it
template <int NA, class LN>
__host__ __device__ inline CPR_AI bool fused_races_due(const LN (&L)[NA], const LaneMem& M) {
  return L[0].qn > M.rq_cap - NA * M.wave;
}

template <int NA, class LN>
__host__ __device__ inline CPR_AI void fused_races_settle(LN (&L)[NA], const LaneMem& M) {
  const int32_t fl = M.rflag[M.lane];
  M.rflag[M.lane] = 0;
  L[0].qn = 0;
#pragma unroll
  for (int i = 0; i < NA; ++i) {
    L[i].status |= ((fl >> (2 * i)) & 1) ? ST_TIE : 0u;
    L[i].status |= ((fl >> (2 * i)) & 2) ? ST_RACE_REDO : 0u;
  }
}

template <int NA, class St, class LN>
__host__ __device__ inline CPR_AI void fused_verify_races(LN (&L)[NA], const NakParams& P,
                                                          const St& S, const LaneMem& M) {
  races_publish(S, M);
  wave_lds_order();
  races_check<St, 2, NA, LN>(L[0], P, S, M);
  wave_lds_order();
  fused_races_settle<NA>(L, M);
}

// one gym step of every point with the built-in policy POL (run_gym's loop body), in two
// halves around the activation's counter block: up to the races' list ...
template <int POL, int NA, int ARR, class St, class LN>
__host__ __device__ inline CPR_AI void fused_step_pre(LN (&L)[NA], const NakParams& P,
                                                      const St& S, const LaneMem& M) {
#pragma unroll
  for (int i = 0; i < NA; ++i) {
    if constexpr (LN::PK && POL >= P_HONEST && POL <= P_SM1) {
      // packed tips: the policy's decisions as flags, no action code (policy_flags)
      int32_t h, a, dd, ev;
      L[i].observe(&h, &a, &dd, &ev);
      const PolicyFlags f = policy_flags<POL>(h, a);
      L[i].apply_flags(f.adopt, f.relx, f.ovr);
    } else {
      L[i].apply(L[i].template policy_action<POL>(P));
    }
    L[i].template resolve<St, 0, ARR ? 2 : 1>(P, S, M);
  }
  if constexpr (ARR != 0) fused_enqueue_races<NA>(L, M);
}
// ... and the activation from block w on
template <int NA, int ARR, class St, class LN>
__host__ __device__ inline CPR_AI void fused_step_post(LN (&L)[NA], const NakParams& P,
                                                       const St& S, const LaneMem& M,
                                                       const uint64_t (&t_att)[NA],
                                                       const Words4& w) {
  fused_activate_w<NA, ARR>(L, P, S, M, t_att, w);
  if constexpr (ARR != 0) {
    // the lanes of the wave verify together once the wave's list is nearly full
    if (fused_races_due<NA>(L, M)) fused_verify_races<NA>(L, P, S, M);
  }
}
template <int POL, int NA, int ARR, class St, class LN>
__host__ __device__ inline CPR_AI void fused_step(LN (&L)[NA], const NakParams& P,
                                                  const St& S, const LaneMem& M,
                                                  const uint64_t (&t_att)[NA]) {
  fused_step_pre<POL, NA, ARR>(L, P, S, M);
  fused_step_post<NA, ARR>(L, P, S, M, t_att, S.block((uint32_t)L[0].k, TAG_ACT));
}

// ---- lane groups: G adjacent lanes of a wave (aligned: lanes g0 .. g0 + G - 1, g0 a multiple
// of G) run the same episode, each with NA points of its own. The TAG_ACT block of an
// activation is the same for all of them, so each lane computes one block per G activations
// and the group passes them round: whenever the activation count k (the same in every lane
// of a wave) is a multiple of G, lane g of the group computes the block of activation k + g
// into `held`; at activation k every lane takes the block lane k mod G holds. Blocks past
// the episode's last activation are computed for nothing. The exchange runs at the top of
// an activation, where the wave is converged; the lanes of a group share their episode
// index, so they enter and leave the episode loop together and no exchange reads a lane
// that is not there.

// the held block of lane g of a group at activation count k
template <int G, class St>
__host__ __device__ inline CPR_AI void group_fill(Words4& held, const St& S, uint32_t k,
                                                  int32_t g) {
  if ((k & (uint32_t)(G - 1)) == 0u) held = S.block(k + (uint32_t)g, TAG_ACT);
}

#if defined(__HIP_DEVICE_COMPILE__)
// The exchange: ds_bpermute_b32 from lane g0 + k mod G, four LDS-pipe operations and no
// VALU. Two DPP forms (a quad_perm broadcast with a rotate of the held blocks; an immediate
// quad_perm broadcast chosen by a scalar branch on k mod G) measured the same and were
// taken out again (DESIGN.md "Lane groups").
// k: the activation count, wave-uniform (in a scalar register); lane: the lane in its wave
template <int G>
__device__ inline CPR_AI Words4 group_take(const Words4& held, uint32_t k, int32_t lane) {
  static_assert(G == 2 || G == 4 || G == 8, "lane groups of 2, 4 or 8");
  const uint32_t r = k & (uint32_t)(G - 1);
  const int src = (int)((((uint32_t)lane & ~(uint32_t)(G - 1)) | r) << 2);
  Words4 w;
  w.w0 = (uint32_t)__builtin_amdgcn_ds_bpermute(src, (int)held.w0);
  w.w1 = (uint32_t)__builtin_amdgcn_ds_bpermute(src, (int)held.w1);
  w.w2 = (uint32_t)__builtin_amdgcn_ds_bpermute(src, (int)held.w2);
  w.w3 = (uint32_t)__builtin_amdgcn_ds_bpermute(src, (int)held.w3);
  return w;
}

// the block of the lane's next activation (G = 1: its own)
template <int G, int NA, class St, class LN>
__device__ inline CPR_AI Words4 group_block(const LN (&L)[NA], const St& S, Words4& held,
                                            int32_t lane) {
  if constexpr (G == 1) {
    return S.block((uint32_t)L[0].k, TAG_ACT);
  } else {
    const uint32_t k = (uint32_t)__builtin_amdgcn_readfirstlane(L[0].k);
    group_fill<G>(held, S, k, lane & (G - 1));
    return group_take<G>(held, k, lane);
  }
}
#else
// the host pass over the kernel's body only needs the name (tests/native_lane_groups models
// a group with group_fill and an exchange of its own)
template <int G, int NA, class St, class LN>
__host__ __device__ inline Words4 group_block(const LN (&L)[NA], const St& S, Words4&,
                                              int32_t) {
  return S.block((uint32_t)L[0].k, TAG_ACT);
}
#endif

}  // namespace cpr
