// TEST INFRASTRUCTURE ONLY. The trimmed step of the fused lanes over packed tips
// (cpr_amd/csrc/nakamoto_lane.h: policy_flags, apply_flags with the step's one released tip,
// no capacity test; nak_fused.h fused_step) beside single lanes over BRef tips that take the
// long way, host build.
// (a) policy_flags<POL>(h, a) against the decoding of nak_policy's action for the four
//     built-in policies and every h, a in 0..40, both observation events; exactly one of
//     adopt / match / override / wait holds.
// (b) NakLanePacked, two points per lane, through fused_reset and fused_step with
//     LaneMem::cap_test = false and cap = max_steps + 2 exactly, beside one NakLane per point
//     through policy_action -> apply -> resolve -> activate with the capacity test on, on the
//     same keyed stream. After the reset and after every step every word of NakLane::pack
//     (but the tips' k, which a packed tip does not keep), rw and tinf must be equal, every
//     race a point lists must be in the fused list with the same word, and at the end the
//     heads. ST_DEEP_FORK must never appear on either side. At gamma = .5 the two sides
//     verify their race lists at different steps, so the tie / redo bits are compared once
//     the last verification has run (as tests/native_fused does).
//     Cases: four policies x ARR {0, 1} x points {(alpha .05, .33), (.5, t_att = 2^32: every
//     block the attacker's, so n reaches max_steps + 1 = cap - 1)} x max_steps {1, 16, 62 (cap
//     64, no rounding slack), 300} x delays {1e-9, 1e-3}; every third episode has one clock
//     uniform forced to zero.
// (c) the lane's own host assertions (CPR_HOST_ASSERT in apply_flags, resolve_packed and
//     activate: where released, rhi == pend; the shared tip equals chain_ref(M, rhi) in
//     resolve and chain_ref(M, pend) at activate, with the same select condition; n + 1 <
//     cap) are live in this build and abort the program; they run in every step of (b).
// usage: step_vs_lane [episodes per case]; one JSON line; exit 1 on any mismatch
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>

#ifdef NDEBUG
#error "the lane's host assertions are part of this test"
#endif

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

// ---- (a)

struct FlagCounts {
  long checked = 0, mismatches = 0, adopt = 0, match = 0, override_ = 0, wait = 0;
};

template <int POL>
static void check_flags(FlagCounts& C) {
  for (int32_t h = 0; h <= 40; ++h)
    for (int32_t a = 0; a <= 40; ++a)
      for (int32_t ev = 0; ev < 2; ++ev) {
        const int32_t act = nak_policy(POL, h, a, ev, nullptr, 0);
        const PolicyFlags f = policy_flags<POL>(h, a);
        const bool match = f.relx && !f.ovr, wait = !f.adopt && !f.relx;
        const int one = (f.adopt ? 1 : 0) + (match ? 1 : 0) + (f.ovr ? 1 : 0) + (wait ? 1 : 0);
        const bool ok = f.adopt == (act == A_ADOPT) &&
                        f.relx == (act == A_MATCH || act == A_OVERRIDE) &&
                        f.ovr == (act == A_OVERRIDE) && match == (act == A_MATCH) &&
                        wait == (act == A_WAIT) && one == 1;
        if (!ok) {
          ++C.mismatches;
          fprintf(stderr, "FLAGS pol=%d h=%d a=%d: action %d, flags adopt %d relx %d ovr %d\n", POL,
                  h, a, act, f.adopt, f.relx, f.ovr);
        }
        ++C.checked;
        C.adopt += f.adopt;
        C.match += match;
        C.override_ += f.ovr;
        C.wait += wait;
      }
}

// ---- (b), (c)

struct Counters {
  long episodes = 0, point_steps = 0, mismatches = 0, deep_fork_points = 0, races = 0,
       drains = 0, redo_points = 0, releases = 0, deliveries = 0, adopts = 0,
       inf_episodes = 0, max_private = 0, cap_minus_private_min = 1 << 30;
};

constexpr int NA = 2;
constexpr int kStatusWord = 11;  // NakLane::pack
constexpr int kTip0 = 12;        // NakLane::pack: five tips of (h, ra, k, fork) from here
constexpr uint32_t kLate = ST_TIE | ST_RACE_REDO;  // set by a verification

static bool same(const NakLanePacked& p, const NakLane& r, bool late) {
  uint32_t a[CK_WORDS], b[CK_WORDS];
  p.pack(a);  // unpacks the tips first
  r.pack(b);
  for (int i = 0; i < 5; ++i) a[kTip0 + 4 * i + 2] = b[kTip0 + 4 * i + 2] = 0u;
  if (!late) {
    a[kStatusWord] &= ~kLate;
    b[kStatusWord] &= ~kLate;
  }
  return memcmp(a, b, sizeof(a)) == 0 && p.rw == r.rw;
}

template <int POL, int ARR>
static void run_episode(const NakParams& P0, uint64_t ep, uint32_t zero_at,
                        const uint64_t (&t_att)[NA], Counters& C) {
  constexpr int LZ = ARR ? 2 : 1, TT = ARR ? 2 : 1;
  constexpr int RQF = RQ_LANE + NA - 1;
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
  // a wave of one lane: the fused lane's race list, and one list per single lane
  uint4 rqf[RQF], rqs[NA][RQ_LANE];
  int32_t flagf = 0, flags[NA] = {};
  uint32_t repf[2], reps[NA][2];
  M.rq = rqf;
  M.rq_cap = RQF;
  M.rflag = &flagf;
  M.rep = repf;
  M.lane = 0;
  M.wave = 1;
  LaneMem MS[NA];
  NakParams PS[NA];  // the single lanes' parameters: the point's own threshold
  for (int i = 0; i < NA; ++i) {
    MS[i] = M;  // the capacity test on
    MS[i].rq = rqs[i];
    MS[i].rq_cap = RQ_LANE;
    MS[i].rflag = &flags[i];
    MS[i].rep = reps[i];
    PS[i] = P0;
    PS[i].t_att = t_att[i];
  }
  M.cap_test = false;  // as k_run_episodes_fused
  NakParams PF = P0;
  PF.t_att = ~0ull;  // the fused lane must not read it
  NakLanePacked F[NA];
  NakLane G[NA];
  bool bad = false;
  auto report = [&](const char* where, int64_t s, int i) {
    bad = true;
    fprintf(stderr, "MISMATCH pol=%d arr=%d delta=%g steps=%lld ep=%llu %s %lld point %d: status "
            "packed %u single %u\n", POL, ARR, P0.delta, (long long)P0.max_steps,
            (unsigned long long)ep, where, (long long)s, i, F[i].status, G[i].status);
  };
  fused_reset<NA, ARR>(F, PF, S, M, t_att);
  for (int i = 0; i < NA; ++i) {
    G[i].init();
    G[i].template activate<ZStream, LZ>(PS[i], S, MS[i]);
    if (!same(F[i], G[i], true) || F[0].tinf != G[i].tinf) report("reset", 0, i);
  }
  for (int64_t s = 0; s < P0.max_steps && !bad; ++s) {
    uint32_t want_rw[NA];
    int want_pt[NA], nwant = 0;
    for (int i = 0; i < NA; ++i) {  // run_gym's loop body (kernels.hip)
      const NakLane::Draw dr = G[i].template draw<ZStream, LZ>(PS[i], S);
      const int32_t act = G[i].template policy_action<POL>(PS[i]);
      const BRef pub0 = G[i].pub;
      G[i].apply(act);
      C.adopts += act == A_ADOPT ? 1 : 0;
      C.releases += G[i].rhi >= G[i].rlo ? 1 : 0;
      G[i].template resolve<ZStream, 0, TT>(PS[i], S, MS[i]);
      if constexpr (ARR != 0) {
        if (G[i].rw != 0u) {
          want_rw[nwant] = G[i].rw;
          want_pt[nwant++] = i;
        }
        enqueue_race<LZ>(G[i], MS[i]);
      }
      const int32_t pend0 = G[i].pend;
      G[i].template activate<ZStream, LZ>(PS[i], S, MS[i], dr);
      // the pending release became pub (a defender block on top of it or not)
      C.deliveries += pend0 >= 0 && G[i].p0.h + pend0 > pub0.h ? 1 : 0;
      if constexpr (ARR != 0) {
        if (races_due(G[i], MS[i])) verify_races<ZStream, LZ>(G[i], PS[i], S, MS[i]);
      }
    }
    const int32_t qn0 = F[0].qn;
    fused_step<POL, NA, ARR>(F, PF, S, M, t_att);
    C.drains += F[0].qn < qn0 ? 1 : 0;
    C.races += nwant;
    // the races of this step in the fused list: the points' words, in point order (the list
    // keeps them where they were written even when the step went on to verify it)
    for (int j = 0; j < nwant && !bad; ++j) {
      const uint4 e = rqf[qn0 + j];
      if (e.w != want_rw[j] || (int)(e.y >> 1) != want_pt[j]) {
        bad = true;
        fprintf(stderr, "MISMATCH pol=%d delta=%g ep=%llu step %lld: race %d listed as %08x of "
                "point %u, single lane %08x of point %d\n", POL, P0.delta,
                (unsigned long long)ep, (long long)s, j, e.w, e.y >> 1, want_rw[j], want_pt[j]);
      }
    }
    for (int i = 0; i < NA && !bad; ++i) {
      if (!same(F[i], G[i], ARR == 0) || F[0].tinf != G[i].tinf) report("step", s, i);
      if ((F[i].status | G[i].status) & ST_DEEP_FORK) report("deep fork at step", s, i);
      C.max_private = G[i].n > C.max_private ? G[i].n : C.max_private;
      const long room = (long)P0.cap - G[i].n;
      C.cap_minus_private_min = room < C.cap_minus_private_min ? room : C.cap_minus_private_min;
    }
    C.point_steps += NA;
  }
  if constexpr (ARR != 0) {
    // the last verification, as at the end of the kernels' episode loop
    fused_verify_races<NA>(F, PF, S, M);
    for (int i = 0; i < NA; ++i) {
      verify_races<ZStream, LZ>(G[i], PS[i], S, MS[i]);
      C.redo_points += (G[i].status & ST_RACE_REDO) ? 1 : 0;
      if (!bad && !same(F[i], G[i], true)) report("end", 0, i);
    }
  }
  for (int i = 0; i < NA && !bad; ++i) {
    const BRef hp = F[i].head(PF, M), hr = G[i].head(PS[i], MS[i]);
    if (hp.h != hr.h || hp.ra != hr.ra || hp.fork != hr.fork) {
      bad = true;
      fprintf(stderr, "MISMATCH pol=%d arr=%d ep=%llu head of point %d: packed (%d, %d) single "
              "(%d, %d)\n", POL, ARR, (unsigned long long)ep, i, hp.h, hp.ra, hr.h, hr.ra);
    }
  }
  ++C.episodes;
  C.mismatches += bad ? 1 : 0;
  C.inf_episodes += zero_at <= (uint32_t)P0.max_steps ? 1 : 0;
  for (int i = 0; i < NA; ++i)
    C.deep_fork_points += ((F[i].status | G[i].status) & ST_DEEP_FORK) ? 1 : 0;
}

template <int POL, int ARR>
static void run_case(double delta, int steps, int episodes, Counters& C) {
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
  P.cap = steps + 2;  // exactly what the fused kernels' launcher asks for, no slack
  if (!lazy_clock_ok(P)) {
    fprintf(stderr, "lazy clock not applicable: delta %g steps %d\n", delta, steps);
    exit(2);
  }
  P.u_lazy = lazy_threshold(P);
  const uint64_t pairs[2][NA] = {
      {oracle::alpha_threshold(0.05), oracle::alpha_threshold(0.33)},
      {oracle::alpha_threshold(0.5), 1ull << 32}};  // 2^32: above every draw
  for (int pr = 0; pr < 2; ++pr)
    for (int e = 0; e < episodes; ++e) {
      const uint64_t ep = 9000 + (uint64_t)e + 1000ull * (uint64_t)(pr + 2 * ARR) +
                          100000ull * (uint64_t)steps;
      const uint32_t z = e % 3 == 2 ? mix(ep, steps) % (uint32_t)steps : 0xffffffffu;
      run_episode<POL, ARR>(P, ep, z, pairs[pr], C);
    }
}

template <int POL, int ARR>
static void run_policy(int episodes, Counters& C) {
  for (double delta : {1e-9, 1e-3})
    for (int steps : {1, 16, 62, 300}) run_case<POL, ARR>(delta, steps, episodes, C);
}

template <int ARR>
static int run_all(const char* name, int episodes) {
  Counters C;
  run_policy<P_HONEST, ARR>(episodes, C);
  run_policy<P_SIMPLE, ARR>(episodes, C);
  run_policy<P_ES2014, ARR>(episodes, C);
  run_policy<P_SM1, ARR>(episodes, C);
  printf("%s{\"episodes\": %ld, \"point_steps\": %ld, \"mismatches\": %ld, "
         "\"deep_fork_points\": %ld, \"races\": %ld, \"drains\": %ld, \"redo_points\": %ld, "
         "\"releases\": %ld, \"deliveries\": %ld, \"adopts\": %ld, \"inf_clock_episodes\": %ld, "
         "\"max_private\": %ld, \"cap_minus_private_min\": %ld}",
         name, C.episodes, C.point_steps, C.mismatches, C.deep_fork_points, C.races, C.drains,
         C.redo_points, C.releases, C.deliveries, C.adopts, C.inf_episodes, C.max_private,
         C.cap_minus_private_min);
  return C.mismatches ? 1 : 0;
}

int main(int argc, char** argv) {
  const int episodes = argc > 1 ? atoi(argv[1]) : 6;
  FlagCounts FC;
  check_flags<P_HONEST>(FC);
  check_flags<P_SIMPLE>(FC);
  check_flags<P_ES2014>(FC);
  check_flags<P_SM1>(FC);
  printf("{\"flags\": {\"checked\": %ld, \"mismatches\": %ld, \"adopt\": %ld, \"match\": %ld, "
         "\"override\": %ld, \"wait\": %ld}", FC.checked, FC.mismatches, FC.adopt, FC.match,
         FC.override_, FC.wait);
  int rc = FC.mismatches ? 1 : 0;
  rc |= run_all<0>(", \"gamma0\": ", episodes);
  rc |= run_all<1>(", \"gamma05\": ", episodes);
  printf("}\n");
  return rc;
}
