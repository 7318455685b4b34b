// TEST INFRASTRUCTURE ONLY. The multi-point lane of k_run_episodes_fused
// (cpr_amd/csrc/nak_fused.h: NA sweep points that share every draw of one episode) beside NA
// single lanes as the one-point timed summary kernels configure them (no block times, lazy
// clock, ties by rule, d = 2; gamma = 0: LZ = 1; gamma = .5: LZ = 2 with deferred races), on
// the same keyed stream and with the same actions, host build. After the reset and after
// every step, every state word (NakLane::pack) and the lazy clock's tinf of point i must equal
// single lane i's. At gamma = 0 that includes the status bits. At gamma = .5 the fused lane
// and the single lanes verify their race lists at different steps (the fused list holds all
// points' races; a wave of one lane is emulated), so the tie / redo bits are compared once
// the last verification has run, and the overlap bit at every step.
// Every fifth episode has one clock uniform forced to zero (delay +inf).
// usage: fused_vs_single [episodes per case]; one JSON line; exit 1 on any mismatch
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "../../cpr_amd/csrc/nak_fused.h"
#include "../../oracle/src/keyed_stream.h"

using namespace cpr;

// the keyed stream with activation `zero_at`'s clock uniform forced to 0
struct ZStream : Stream {
  uint32_t zero_at = 0xffffffffu;
  Words4 block(uint32_t idx, uint32_t tag) const {
    Words4 w = Stream::block(idx, tag);
    if (tag == TAG_ACT && idx == zero_at) w.w2 = w.w3 = 0u;
    return w;
  }
  double clock(uint32_t j, double ev) const {
    return j == zero_at ? (-1.0 * ev) * cpr_log(0.0) : Stream::clock(j, ev);
  }
  uint64_t act_u(uint32_t j, uint64_t t_att, int32_t d, int32_t* m) const {
    const uint64_t u = Stream::act_u(j, t_att, d, m);
    return j == zero_at ? 0ull : u;
  }
};

static uint32_t mix(uint64_t a, uint64_t b) {
  uint64_t x = a * 0x9E3779B97F4A7C15ull ^ (b + 0x632BE59BD9B4E019ull);
  x ^= x >> 31;
  x *= 0xD6E8FEB86659FD93ull;
  x ^= x >> 32;
  return (uint32_t)x;
}

struct Counters {
  long episodes = 0, point_steps = 0, mismatches = 0, overlap_points = 0, inf_episodes = 0,
       exact_entries = 0, split_episodes = 0, races = 0, redo_points = 0, drains = 0;
};

constexpr int kStatusWord = 11;  // NakLane::pack
constexpr uint32_t kLate = ST_TIE | ST_RACE_REDO;  // set by a verification

static const double kAlphas[6] = {0.05, 0.25, 0.35, 0.45, 0.5, 0.10};

// late: the bits a verification sets are compared too
static bool same(const NakLane& a, const NakLane& b, bool late = true) {
  uint32_t ca[CK_WORDS], cb[CK_WORDS];
  a.pack(ca);
  b.pack(cb);
  if (!late) {
    ca[kStatusWord] &= ~kLate;
    cb[kStatusWord] &= ~kLate;
  }
  return memcmp(ca, cb, sizeof(ca)) == 0 && a.tinf == b.tinf;
}

template <int POL, int NA, int ARR>
static void run_episode(const NakParams& P0, uint64_t ep, uint32_t zero_at, int a0, Counters& C) {
  const uint64_t seed = 0x5eed0000ull;
  ZStream S;
  S.k0 = (uint32_t)seed;
  S.k1 = (uint32_t)(seed >> 32);
  S.e0 = (uint32_t)ep;
  S.e1 = (uint32_t)(ep >> 32);
  S.zero_at = zero_at;
  LaneMem M;
  M.ring = nullptr;
  M.spill = nullptr;
  M.ring_stride = M.spill_stride = 0;
  M.cap = P0.cap;
  M.replay.nodes = nullptr;
  M.replay.masks = nullptr;
  M.times = false;
  M.d2 = true;
  // deferred races: a wave of one lane; the fused lane's list, and one list per single lane
  constexpr int LZ = ARR ? 2 : 1, TT = ARR ? 2 : 1;
  constexpr int RQF = RQ_LANE + NA - 1;
  uint4 rqf[RQF], rqs[NA][RQ_LANE];
  int32_t flagf = 0, flags[NA] = {};
  uint32_t repf[2], reps[NA][2];
  LaneMem MS[NA];
  M.rq = rqf;
  M.rq_cap = RQF;
  M.rflag = &flagf;
  M.rep = repf;
  M.lane = 0;
  M.wave = 1;
  for (int i = 0; i < NA; ++i) {
    MS[i] = M;
    MS[i].rq = rqs[i];
    MS[i].rq_cap = RQ_LANE;
    MS[i].rflag = &flags[i];
    MS[i].rep = reps[i];
  }
  uint64_t t_att[NA];
  NakParams PS[NA];  // the single lanes' parameters: the point's own threshold
  for (int i = 0; i < NA; ++i) {
    t_att[i] = oracle::alpha_threshold(kAlphas[(a0 + i) % 6]);
    PS[i] = P0;
    PS[i].t_att = t_att[i];
  }
  NakParams PF = P0;
  PF.t_att = ~0ull;  // the fused lane must not read it
  NakLane F[NA], G[NA];
  bool bad = false;
  fused_reset<NA, ARR>(F, PF, S, M, t_att);
  for (int i = 0; i < NA; ++i) {
    G[i].init();
    G[i].template activate<ZStream, LZ>(PS[i], S, MS[i]);
    bad |= !same(F[i], G[i]);
  }
  for (int64_t s = 0; s < P0.max_steps && !bad; ++s) {
    const uint32_t uh = (uint32_t)(S.block((uint32_t)F[0].k, TAG_ACT).w2 >> 5);
    C.exact_entries += ((uh - 1u) >= (lazy_hi(P0.u_lazy) - 1u) || F[0].tinf) ? 1 : 0;
    for (int i = 0; i < NA; ++i) {  // run_gym's loop body (kernels.hip)
      const NakLane::Draw dr = G[i].template draw<ZStream, LZ>(PS[i], S);
      G[i].apply(G[i].template policy_action<POL>(PS[i]));
      G[i].template resolve<ZStream, 0, TT>(PS[i], S, MS[i]);
      if constexpr (ARR != 0) {
        C.races += G[i].rw != 0u ? 1 : 0;
        enqueue_race<LZ>(G[i], MS[i]);
      }
      G[i].template activate<ZStream, LZ>(PS[i], S, MS[i], dr);
      if constexpr (ARR != 0) {
        if (races_due(G[i], MS[i])) verify_races<ZStream, LZ>(G[i], PS[i], S, MS[i]);
      }
    }
    const int32_t qn0 = F[0].qn;
    fused_step<POL, NA, ARR>(F, PF, S, M, t_att);
    C.drains += F[0].qn < qn0 ? 1 : 0;
    for (int i = 0; i < NA; ++i)
      if (!same(F[i], G[i], ARR == 0)) {
        bad = true;
        fprintf(stderr, "MISMATCH na=%d pol=%d delta=%g ep=%llu step %lld point %d: status fused "
                "%u single %u\n", NA, POL, P0.delta, (unsigned long long)ep, (long long)s, i,
                F[i].status, G[i].status);
      }
    C.point_steps += NA;
  }
  if constexpr (ARR != 0) {
    // the last verification, as at the end of the kernels' episode loop
    fused_verify_races<NA>(F, PF, S, M);
    for (int i = 0; i < NA; ++i) {
      verify_races<ZStream, LZ>(G[i], PS[i], S, MS[i]);
      C.redo_points += (G[i].status & ST_RACE_REDO) ? 1 : 0;
      if (!bad && !same(F[i], G[i])) {
        bad = true;
        fprintf(stderr, "MISMATCH na=%d pol=%d delta=%g ep=%llu at the end, point %d: status fused "
                "%u single %u\n", NA, POL, P0.delta, (unsigned long long)ep, i, F[i].status,
                G[i].status);
      }
    }
  }
  ++C.episodes;
  C.mismatches += bad ? 1 : 0;
  C.inf_episodes += zero_at <= (uint32_t)P0.max_steps ? 1 : 0;
  int ov = 0;
  for (int i = 0; i < NA; ++i) ov += (G[i].status & ST_OVERLAP) ? 1 : 0;
  C.overlap_points += ov;
  C.split_episodes += (ov > 0 && ov < NA) ? 1 : 0;  // some points flagged, their siblings not
}

template <int POL, int NA, int ARR>
static void run_case(double delta, int steps, int episodes, Counters& C) {
  if constexpr (NA <= (ARR ? CPR_NAK_FUSE_MAX_ARR : CPR_NAK_FUSE_MAX)) {
    NakParams P{};
    P.d = 2;
    P.ev = 1.0;
    P.delta = delta;
    P.dmax = ARR ? delta : __builtin_inf();  // the gym's gamma = .5 / gamma = 0 networks
    P.arrive = ARR;
    P.max_steps = steps;
    P.max_progress = __builtin_inf();
    P.max_time = __builtin_inf();
    P.policy = POL;
    P.cap = steps + 64 < 4096 ? steps + 64 : 4096;  // release indices fit a list entry
    if (!lazy_clock_ok(P)) {
      fprintf(stderr, "lazy clock not applicable: delta %g steps %d\n", delta, steps);
      exit(2);
    }
    P.u_lazy = lazy_threshold(P);
    for (int e = 0; e < episodes; ++e) {
      const uint64_t ep = 1000 + (uint64_t)e + 100000ull * (uint64_t)(NA + 8 * ARR);
      const uint32_t z = e % 5 == 4 ? mix(ep, steps) % (uint32_t)steps : 0xffffffffu;
      run_episode<POL, NA, ARR>(P, ep, z, e + NA, C);
    }
  }
}

template <int POL, int ARR>
static void run_policy(int episodes, Counters& C) {
  for (double delta : {1e-9, 1e-3, 0.05}) {
    run_case<POL, 2, ARR>(delta, 300, episodes, C);
    run_case<POL, 3, ARR>(delta, 300, episodes, C);
    run_case<POL, 4, ARR>(delta, 300, episodes, C);
    run_case<POL, 5, ARR>(delta, 300, episodes, C);
  }
  // the lazy clock's longest episode, once per group size
  run_case<POL, 2, ARR>(1e-3, 16384, 1, C);
  run_case<POL, ARR ? CPR_NAK_FUSE_MAX_ARR : CPR_NAK_FUSE_MAX, ARR>(1e-3, 16384, 1, C);
}

static int report(const char* name, int fuse_max, const Counters& C) {
  printf("%s{\"fuse_max\": %d, \"episodes\": %ld, \"point_steps\": %ld, \"mismatches\": %ld, "
         "\"exact_branch_entries\": %ld, \"overlap_points\": %ld, \"split_episodes\": %ld, "
         "\"inf_clock_episodes\": %ld, \"races\": %ld, \"redo_points\": %ld, \"drains\": %ld}",
         name, fuse_max, C.episodes, C.point_steps, C.mismatches, C.exact_entries,
         C.overlap_points, C.split_episodes, C.inf_episodes, C.races, C.redo_points, C.drains);
  return C.mismatches ? 1 : 0;
}

template <int ARR>
static void run_all(int episodes, Counters& C) {
  run_policy<P_HONEST, ARR>(episodes, C);
  run_policy<P_SIMPLE, ARR>(episodes, C);
  run_policy<P_ES2014, ARR>(episodes, C);
  run_policy<P_SM1, ARR>(episodes, C);
}

int main(int argc, char** argv) {
  const int episodes = argc > 1 ? atoi(argv[1]) : 20;
  Counters C0, C1;
  run_all<0>(episodes, C0);
  run_all<1>(episodes, C1);
  int rc = report("{\"gamma0\": ", CPR_NAK_FUSE_MAX, C0);
  rc |= report(", \"gamma05\": ", CPR_NAK_FUSE_MAX_ARR, C1);
  printf("}\n");
  return rc;
}
