// TEST INFRASTRUCTURE ONLY. A lane group of k_run_episodes_fused (cpr_amd/csrc/nak_fused.h
// "lane groups": G lanes that run one episode, NA sweep points each, and pass the TAG_ACT
// blocks round) beside NA * G single lanes as the one-point timed summary kernels configure
// them, on the same keyed stream and with the same actions, host build.
// The group is G lane objects stepped in lockstep: every lane runs the first half of the step
// (fused_step_pre), then every lane refills its held block where the activation count is a
// multiple of G (group_fill, the kernel's own), then the exchange (a function over the array
// of held blocks) hands every lane the block of lane k mod G, then every lane runs the second
// half (fused_step_post). After the reset and after every step, every state word
// (NakLane::pack) and the lazy clock's tinf of every point must equal its single lane's; at
// gamma = .5 every lane verifies its own list (a wave of one lane is emulated), so the tie /
// redo bits are compared once the last verification has run, and the overlap bit at every step.
// Every fifth episode has one clock uniform forced to zero (delay +inf).
// usage: lane_groups_vs_single [episodes per case]; one JSON line; exit 1 on any mismatch
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

// the same stream, counting the TAG_ACT blocks it computes: what group_fill draws from
struct CountStream : ZStream {
  long* n_act = nullptr;
  Words4 block(uint32_t idx, uint32_t tag) const {
    if (tag == TAG_ACT) ++*n_act;
    return ZStream::block(idx, tag);
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
       exact_entries = 0, split_episodes = 0, split_lanes = 0, races = 0, redo_points = 0,
       drains = 0, blocks = 0, blocks_expected = 0, block_errors = 0;
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

// the exchange: at activation count k every lane of the group takes the block lane k mod G
// holds
template <int G>
static Words4 exchange(const Words4 (&held)[G], uint32_t k) {
  return held[k & (uint32_t)(G - 1)];
}

// one lane of a group: its points' states, its race list (a wave of one lane) and its block
template <int NA>
struct GroupLane {
  NakLane F[NA];
  LaneMem M;
  uint64_t t_att[NA];
  uint4 rq[RQ_LANE + NA - 1];
  int32_t flag = 0;
  uint32_t rep[2];
  long blocks = 0;
};

template <int POL, int NA, int ARR, int G>
static void run_episode(const NakParams& P0, uint64_t ep, uint32_t zero_at, int a0, Counters& C) {
  constexpr int NP = NA * G;
  const uint64_t seed = 0x5eed0000ull;
  ZStream S;
  S.k0 = (uint32_t)seed;
  S.k1 = (uint32_t)(seed >> 32);
  S.e0 = (uint32_t)ep;
  S.e1 = (uint32_t)(ep >> 32);
  S.zero_at = zero_at;
  LaneMem M0;
  M0.ring = nullptr;
  M0.spill = nullptr;
  M0.ring_stride = M0.spill_stride = 0;
  M0.cap = P0.cap;
  M0.replay.nodes = nullptr;
  M0.replay.masks = nullptr;
  M0.times = false;
  M0.d2 = true;
  M0.lane = 0;
  M0.wave = 1;
  constexpr int LZ = ARR ? 2 : 1, TT = ARR ? 2 : 1;
  // the group
  static GroupLane<NA> GL[G];
  Words4 held[G];
  CountStream CS[G];
  for (int g = 0; g < G; ++g) {
    GL[g].M = M0;
    GL[g].M.rq = GL[g].rq;
    GL[g].M.rq_cap = RQ_LANE + NA - 1;
    GL[g].flag = 0;
    GL[g].M.rflag = &GL[g].flag;
    GL[g].M.rep = GL[g].rep;
    GL[g].blocks = 0;
    static_cast<ZStream&>(CS[g]) = S;
    CS[g].n_act = &GL[g].blocks;
    held[g] = Words4{0u, 0u, 0u, 0u};
    for (int i = 0; i < NA; ++i)
      GL[g].t_att[i] = oracle::alpha_threshold(kAlphas[(a0 + g * NA + i) % 6]);
  }
  // the single lanes: point p = g * NA + i with its own threshold and its own list
  static uint4 rqs[NP][RQ_LANE];
  int32_t flags[NP] = {};
  uint32_t reps[NP][2];
  LaneMem MS[NP];
  NakParams PS[NP];
  NakLane Q[NP];
  for (int p = 0; p < NP; ++p) {
    MS[p] = M0;
    MS[p].rq = rqs[p];
    MS[p].rq_cap = RQ_LANE;
    MS[p].rflag = &flags[p];
    MS[p].rep = reps[p];
    PS[p] = P0;
    PS[p].t_att = GL[p / NA].t_att[p % NA];
  }
  NakParams PF = P0;
  PF.t_att = ~0ull;  // the group's lanes must not read it
  bool bad = false;
  long activations = 0;
  // an activation of the whole group: fill, exchange, then the rest of every lane's step
  auto activation = [&](bool reset) {
    const uint32_t k = (uint32_t)GL[0].F[0].k;
    for (int g = 1; g < G; ++g) bad |= (uint32_t)GL[g].F[0].k != k;  // lockstep
    for (int g = 0; g < G; ++g) group_fill<G>(held[g], CS[g], k, g);
    const Words4 w = exchange<G>(held, k);
    const Words4 own = S.block(k, TAG_ACT);
    if (memcmp(&w, &own, sizeof(w)) != 0) {
      ++C.block_errors;
      bad = true;
    }
    for (int g = 0; g < G; ++g) {
      if (reset)
        fused_activate_w<NA, ARR>(GL[g].F, PF, S, GL[g].M, GL[g].t_att, w);
      else
        fused_step_post<NA, ARR>(GL[g].F, PF, S, GL[g].M, GL[g].t_att, w);
    }
    ++activations;
  };
  for (int g = 0; g < G; ++g)
    for (int i = 0; i < NA; ++i) GL[g].F[i].init();
  activation(true);
  for (int p = 0; p < NP; ++p) {
    Q[p].init();
    Q[p].template activate<ZStream, LZ>(PS[p], S, MS[p]);
    bad |= !same(GL[p / NA].F[p % NA], Q[p]);
  }
  for (int64_t s = 0; s < P0.max_steps && !bad; ++s) {
    const uint32_t uh = (uint32_t)(S.block((uint32_t)Q[0].k, TAG_ACT).w2 >> 5);
    C.exact_entries += ((uh - 1u) >= (lazy_hi(P0.u_lazy) - 1u) || Q[0].tinf) ? 1 : 0;
    for (int p = 0; p < NP; ++p) {  // run_gym's loop body (kernels.hip)
      const NakLane::Draw dr = Q[p].template draw<ZStream, LZ>(PS[p], S);
      Q[p].apply(Q[p].template policy_action<POL>(PS[p]));
      Q[p].template resolve<ZStream, 0, TT>(PS[p], S, MS[p]);
      if constexpr (ARR != 0) {
        C.races += Q[p].rw != 0u ? 1 : 0;
        enqueue_race<LZ>(Q[p], MS[p]);
      }
      Q[p].template activate<ZStream, LZ>(PS[p], S, MS[p], dr);
      if constexpr (ARR != 0) {
        if (races_due(Q[p], MS[p])) verify_races<ZStream, LZ>(Q[p], PS[p], S, MS[p]);
      }
    }
    int32_t qn0[G];
    for (int g = 0; g < G; ++g) {
      qn0[g] = GL[g].F[0].qn;
      fused_step_pre<POL, NA, ARR>(GL[g].F, PF, S, GL[g].M);
    }
    activation(false);
    for (int g = 0; g < G; ++g) C.drains += GL[g].F[0].qn < qn0[g] ? 1 : 0;
    for (int p = 0; p < NP; ++p)
      if (!same(GL[p / NA].F[p % NA], Q[p], ARR == 0)) {
        bad = true;
        fprintf(stderr, "MISMATCH g=%d na=%d pol=%d delta=%g ep=%llu step %lld point %d: status "
                "group %u single %u\n", G, NA, POL, P0.delta, (unsigned long long)ep,
                (long long)s, p, GL[p / NA].F[p % NA].status, Q[p].status);
      }
    C.point_steps += NP;
  }
  if constexpr (ARR != 0) {
    // the last verification, as at the end of the kernels' episode loop
    for (int g = 0; g < G; ++g) fused_verify_races<NA>(GL[g].F, PF, S, GL[g].M);
    for (int p = 0; p < NP; ++p) {
      verify_races<ZStream, LZ>(Q[p], PS[p], S, MS[p]);
      C.redo_points += (Q[p].status & ST_RACE_REDO) ? 1 : 0;
      if (!bad && !same(GL[p / NA].F[p % NA], Q[p])) {
        bad = true;
        fprintf(stderr, "MISMATCH g=%d na=%d pol=%d delta=%g ep=%llu at the end, point %d: status "
                "group %u single %u\n", G, NA, POL, P0.delta, (unsigned long long)ep, p,
                GL[p / NA].F[p % NA].status, Q[p].status);
      }
    }
  }
  // every lane computed one block per G activations, rounded up
  for (int g = 0; g < G; ++g) {
    C.blocks += GL[g].blocks;
    C.blocks_expected += (activations + G - 1) / G;
    if (!bad && GL[g].blocks != (activations + G - 1) / G) {
      bad = true;
      ++C.block_errors;
    }
  }
  if (!bad && activations != P0.max_steps + 1) bad = true;
  ++C.episodes;
  C.mismatches += bad ? 1 : 0;
  C.inf_episodes += zero_at <= (uint32_t)P0.max_steps ? 1 : 0;
  int ov = 0, lanes_ov = 0;
  for (int g = 0; g < G; ++g) {
    int o = 0;
    for (int i = 0; i < NA; ++i) o += (Q[g * NA + i].status & ST_OVERLAP) ? 1 : 0;
    ov += o;
    lanes_ov += o > 0 ? 1 : 0;
  }
  C.overlap_points += ov;
  C.split_episodes += (ov > 0 && ov < NP) ? 1 : 0;  // some points flagged, their siblings not
  C.split_lanes += (lanes_ov > 0 && lanes_ov < G) ? 1 : 0;  // ... some lanes of a group, not all
}

template <int POL, int NA, int ARR, int G>
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
  if (!lazy_clock_ok(P)) {
    fprintf(stderr, "lazy clock not applicable: delta %g steps %d\n", delta, steps);
    exit(2);
  }
  P.u_lazy = lazy_threshold(P);
  for (int e = 0; e < episodes; ++e) {
    const uint64_t ep =
        1000 + (uint64_t)e + 100000ull * (uint64_t)(NA + 8 * ARR + 16 * G) + 7ull * steps;
    const uint32_t z = e % 5 == 4 ? mix(ep, steps) % (uint32_t)steps : 0xffffffffu;
    run_episode<POL, NA, ARR, G>(P, ep, z, e + NA, C);
  }
}

template <int POL, int NA, int ARR, int G>
static void run_shape(int episodes, Counters& C) {
  for (double delta : {1e-9, 1e-3, 0.05})
    for (int steps : {299, 300, 301, 302})  // activations mod G: every residue
      run_case<POL, NA, ARR, G>(delta, steps, episodes, C);
  // the lazy clock's longest episode
  if (POL == P_SM1) run_case<POL, NA, ARR, G>(1e-3, 16384, 1, C);
}

template <int POL, int ARR>
static void run_policy(int episodes, Counters& C) {
  if constexpr (ARR == 0) {
    run_shape<POL, 2, 0, 2>(episodes, C);
    run_shape<POL, 2, 0, 4>(episodes, C);
    run_shape<POL, 5, 0, 2>(episodes, C);
    run_shape<POL, 5, 0, 4>(episodes, C);
  } else {
    run_shape<POL, 2, 1, 2>(episodes, C);
    run_shape<POL, 2, 1, 4>(episodes, C);
  }
}

static int report(const char* name, const Counters& C) {
  printf("%s{\"episodes\": %ld, \"point_steps\": %ld, \"mismatches\": %ld, "
         "\"exact_branch_entries\": %ld, \"overlap_points\": %ld, \"split_episodes\": %ld, "
         "\"split_lanes\": %ld, \"inf_clock_episodes\": %ld, \"races\": %ld, "
         "\"redo_points\": %ld, \"drains\": %ld, \"blocks\": %ld, \"blocks_expected\": %ld, "
         "\"block_errors\": %ld}",
         name, C.episodes, C.point_steps, C.mismatches, C.exact_entries, C.overlap_points,
         C.split_episodes, C.split_lanes, C.inf_episodes, C.races, C.redo_points, C.drains,
         C.blocks, C.blocks_expected, C.block_errors);
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
  const int episodes = argc > 1 ? atoi(argv[1]) : 10;
  Counters C0, C1;
  run_all<0>(episodes, C0);
  run_all<1>(episodes, C1);
  int rc = report("{\"gamma0\": ", C0);
  rc |= report(", \"gamma05\": ", C1);
  printf("}\n");
  return rc;
}
