// TEST INFRASTRUCTURE ONLY. The lane over packed tips (NakLanePacked: h and ra of a tip in
// one word, cpr_amd/csrc/nakamoto_lane.h PTip), as k_run_episodes_fused runs it, beside the
// lane over BRef tips (NakLane), host build: two sweep points per lane, both lanes driven
// through fused_reset, fused_step and fused_verify_races (nak_fused.h) on the same keyed
// stream. After the reset, after every step and after the last verification, every word of
// NakLane::pack except the tips' k (a packed tip keeps none), tinf, esum, qn and rw of every
// point must be equal, and at gamma = .5 every entry of the two race lists; at the end the
// heads as well. The packed lane's own assertions (no h carries into ra) are live in this
// build and abort the program.
// Cases: the four built-in policies x ARR {0, 1} x alphas {(.05, .33), (.5, t_att = 2^32: every
// block the attacker's)} x max_steps {16, 300, 2016, 16384} x delays {1e-9 (ties in ~1e-3 of
// races), 1e-3}; every third episode has one clock uniform forced to zero (delay +inf).
// usage: packed_vs_refs [episodes per case]; one JSON line; exit 1 on any mismatch
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
       races = 0, drains = 0, redo_points = 0, tie_points = 0, deep_fork_points = 0,
       max_height = 0, max_private = 0;
};

constexpr int NA = 2;
constexpr int kTip0 = 12;  // NakLane::pack: five tips of (h, ra, k, fork) from here

static bool same(const NakLanePacked& p, const NakLane& r) {
  uint32_t a[CK_WORDS], b[CK_WORDS];
  p.pack(a);  // unpacks the tips first
  r.pack(b);
  for (int i = 0; i < 5; ++i) a[kTip0 + 4 * i + 2] = b[kTip0 + 4 * i + 2] = 0u;
  return memcmp(a, b, sizeof(a)) == 0 && p.tinf == r.tinf && p.esum == r.esum && p.qn == r.qn &&
         p.rw == r.rw;
}

struct Lists {  // a wave of one lane: the race list, its flag and episode words
  uint4 rq[RQ_LANE + NA - 1];
  int32_t flag = 0;
  uint32_t rep[2];
  void attach(LaneMem& M) {
    M.rq = rq;
    M.rq_cap = RQ_LANE + NA - 1;
    M.rflag = &flag;
    M.rep = rep;
    M.lane = 0;
    M.wave = 1;
  }
};

template <int POL, int ARR>
static void run_episode(const NakParams& P, uint64_t ep, uint32_t zero_at,
                        const uint64_t (&t_att)[NA], Counters& C) {
  const uint64_t seed = 0x5eed0000ull;
  ZStream S;
  S.k0 = (uint32_t)seed;
  S.k1 = (uint32_t)(seed >> 32);
  S.e0 = (uint32_t)ep;
  S.e1 = (uint32_t)(ep >> 32);
  S.zero_at = zero_at;
  LaneMem MP;
  MP.ring = nullptr;
  MP.spill = nullptr;
  MP.ring_stride = MP.spill_stride = 0;
  MP.cap = P.cap;
  MP.replay.nodes = nullptr;
  MP.replay.masks = nullptr;
  MP.times = false;
  MP.d2 = true;
  LaneMem MR = MP;
  Lists lp, lr;
  lp.attach(MP);
  lr.attach(MR);
  NakLanePacked F[NA];
  NakLane G[NA];
  bool bad = false;
  auto check = [&](const char* where, int64_t s) {
    for (int i = 0; i < NA && !bad; ++i)
      if (!same(F[i], G[i])) {
        bad = true;
        fprintf(stderr, "MISMATCH pol=%d arr=%d delta=%g steps=%lld ep=%llu %s %lld point %d: "
                "status packed %u refs %u\n", POL, ARR, P.delta, (long long)P.max_steps,
                (unsigned long long)ep, where, (long long)s, i, F[i].status, G[i].status);
      }
    if (ARR != 0 && !bad) {
      // the two lists: the same races in the same order
      if (memcmp(lp.rq, lr.rq, sizeof(uint4) * (size_t)G[0].qn) != 0) {
        bad = true;
        fprintf(stderr, "MISMATCH pol=%d delta=%g ep=%llu %s %lld: race lists differ\n", POL,
                P.delta, (unsigned long long)ep, where, (long long)s);
      }
    }
  };
  fused_reset<NA, ARR>(F, P, S, MP, t_att);
  fused_reset<NA, ARR>(G, P, S, MR, t_att);
  check("reset", 0);
  for (int64_t s = 0; s < P.max_steps && !bad; ++s) {
    const int32_t qn0 = G[0].qn;
    fused_step<POL, NA, ARR>(F, P, S, MP, t_att);
    fused_step<POL, NA, ARR>(G, P, S, MR, t_att);
    C.drains += G[0].qn < qn0 ? 1 : 0;
    C.races += G[0].qn > qn0 ? G[0].qn - qn0 : 0;
    check("step", s);
    C.point_steps += NA;
    for (int i = 0; i < NA; ++i) {
      const long h = G[i].pub.h > G[i].D.h ? G[i].pub.h : G[i].D.h;
      C.max_height = h > C.max_height ? h : C.max_height;
      C.max_private = G[i].n > C.max_private ? G[i].n : C.max_private;
    }
  }
  if constexpr (ARR != 0) {
    fused_verify_races<NA>(F, P, S, MP);
    fused_verify_races<NA>(G, P, S, MR);
    check("end", 0);
  }
  for (int i = 0; i < NA && !bad; ++i) {
    const BRef hp = F[i].head(P, MP), hr = G[i].head(P, MR);
    if (hp.h != hr.h || hp.ra != hr.ra || hp.fork != hr.fork) {
      bad = true;
      fprintf(stderr, "MISMATCH pol=%d arr=%d ep=%llu head of point %d: packed (%d, %d) refs "
              "(%d, %d)\n", POL, ARR, (unsigned long long)ep, i, hp.h, hp.ra, hr.h, hr.ra);
    }
  }
  ++C.episodes;
  C.mismatches += bad ? 1 : 0;
  C.inf_episodes += zero_at <= (uint32_t)P.max_steps ? 1 : 0;
  for (int i = 0; i < NA; ++i) {
    C.overlap_points += (G[i].status & ST_OVERLAP) ? 1 : 0;
    C.redo_points += (G[i].status & ST_RACE_REDO) ? 1 : 0;
    C.tie_points += (G[i].status & ST_TIE) ? 1 : 0;
    C.deep_fork_points += (G[i].status & ST_DEEP_FORK) ? 1 : 0;
  }
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
  P.cap = steps + 64 < 4096 ? steps + 64 : 4096;  // release indices fit a list entry
  P.t_att = ~0ull;  // the fused lanes must not read it
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
      const uint64_t ep = 7000 + (uint64_t)e + 1000ull * (uint64_t)(pr + 2 * ARR) +
                          100000ull * (uint64_t)steps;
      const uint32_t z = e % 3 == 2 ? mix(ep, steps) % (uint32_t)steps : 0xffffffffu;
      run_episode<POL, ARR>(P, ep, z, pairs[pr], C);
    }
}

template <int POL, int ARR>
static void run_policy(int episodes, Counters& C) {
  for (double delta : {1e-9, 1e-3}) {
    run_case<POL, ARR>(delta, 16, episodes, C);
    run_case<POL, ARR>(delta, 300, episodes, C);
    run_case<POL, ARR>(delta, 2016, episodes / 2 + 1, C);
    run_case<POL, ARR>(delta, 16384, 1, C);
  }
  // the longest episode with a +inf clock draw as well
  run_case<POL, ARR>(1e-3, 16384, 3, C);
}

template <int ARR>
static int run_all(const char* name, int episodes) {
  Counters C;
  run_policy<P_HONEST, ARR>(episodes, C);
  run_policy<P_SIMPLE, ARR>(episodes, C);
  run_policy<P_ES2014, ARR>(episodes, C);
  run_policy<P_SM1, ARR>(episodes, C);
  printf("%s{\"episodes\": %ld, \"point_steps\": %ld, \"mismatches\": %ld, \"overlap_points\": %ld, "
         "\"inf_clock_episodes\": %ld, \"races\": %ld, \"drains\": %ld, \"redo_points\": %ld, "
         "\"tie_points\": %ld, \"deep_fork_points\": %ld, \"max_height\": %ld, "
         "\"max_private\": %ld}",
         name, C.episodes, C.point_steps, C.mismatches, C.overlap_points, C.inf_episodes, C.races,
         C.drains, C.redo_points, C.tie_points, C.deep_fork_points, C.max_height, C.max_private);
  return C.mismatches ? 1 : 0;
}

int main(int argc, char** argv) {
  const int episodes = argc > 1 ? atoi(argv[1]) : 6;
  int rc = run_all<0>("{\"gamma0\": ", episodes);
  rc |= run_all<1>(", \"gamma05\": ", episodes);
  printf("}\n");
  return rc;
}
