// TEST INFRASTRUCTURE ONLY. The lane as the two timed summary-only kernels configure it
// (cpr_amd/csrc/kernels.hip gym_run_fn: no block times, the lazy clock with its high-word
// skip test, the 32-bit miner draw, 32-bit defender masks at d = 2; at gamma = .5 the
// deferred races, verified over an emulated wave's shared list) beside the general eager
// lane (block times, 64-bit masks, every race decided at once, ties by the heap replay) on
// the same keyed stream, host build. After every step the two must show the same
// observation, the same head (h, ra), the same activation count and, at gamma = 0, the same
// status bits; at gamma = .5 the status is compared once the wave's last verification has
// run, and an episode it flags for the eager second pass (ST_RACE_REDO) is discarded, as
// the kernel does. Every draw's miner is also checked against the 64-bit formula written
// out here, alpha = 1 (t_att = 2^32) included.
// usage: summary_lane_vs_eager [short episodes per config] [long episodes per config]
// one JSON line; exit 1 on any mismatch
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../../cpr_amd/csrc/nakamoto_lane.h"
#include "../../oracle/src/keyed_stream.h"

using namespace cpr;

// the keyed stream with activation `zero_at`'s clock uniform forced to 0 (delay +inf)
struct ZStream : Stream {
  uint32_t zero_at = 0xffffffffu;
  double act(uint32_t j, uint64_t t_att, int32_t d, double ev, int32_t* m) const {
    const double dt = Stream::act(j, t_att, d, ev, m);
    return j == zero_at ? (-1.0 * ev) * cpr_log(0.0) : dt;
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
  long episodes = 0, steps = 0, mismatches = 0, miner_mismatches = 0, exact_entries = 0,
       overlaps = 0, ties = 0, redo = 0, inf_eps = 0, races = 0, drains = 0, alpha1_draws = 0;
};

// what is compared after every step
struct View {
  int32_t obs[4], h, ra, k;
  uint32_t status;
  bool same(const View& o, bool with_status) const {
    for (int i = 0; i < 4; ++i)
      if (obs[i] != o.obs[i]) return false;
    return h == o.h && ra == o.ra && k == o.k && (!with_status || status == o.status);
  }
};
static View view(const NakLane& L, const NakParams& P, const LaneMem& M) {
  View v;
  L.observe(&v.obs[0], &v.obs[1], &v.obs[2], &v.obs[3]);
  const BRef hd = L.head(P, M);
  v.h = hd.h;
  v.ra = hd.ra;
  v.k = L.k;
  v.status = L.status & ~(uint32_t)ST_RACE_REDO;
  return v;
}

// the miner of activation j by the 64-bit comparison and product (the stream's definition)
static int32_t miner64(const Stream& S, uint32_t j, uint64_t t_att, int32_t d) {
  const Words4 w = S.block(j, TAG_ACT);
  if ((uint64_t)w.w0 < t_att) return 0;
  return 1 + (int32_t)(((uint64_t)w.w1 * (uint64_t)d) >> 32);
}

struct Cfg {
  double alpha, gamma, delta;
  int d, policy, steps;  // policy 0..3 (nak_policy), 4 = random actions
};

constexpr int W = 4;         // lanes of the emulated wave
constexpr int PER_LANE = 6;  // list entries per lane (RQ_LANE in the kernel)

// one emulated wave: lane i runs episode ep0 + i; D2: the d = 2 kernels (TT != 0)
template <bool ARR, bool D2>
static void run_wave(const Cfg& cf, uint64_t ep0, uint32_t zero_lane0, Counters& C) {
  constexpr int LZ = ARR ? 2 : 1;
  constexpr int TT = ARR ? 2 : (D2 ? 1 : 0);
  NakParams P{};
  P.t_att = cf.alpha >= 1.0 ? (1ull << 32) : oracle::alpha_threshold(cf.alpha);
  P.d = cf.d;
  P.ev = 1.0;
  P.delta = cf.delta;
  P.dmax = ARR ? cf.delta : __builtin_inf();  // the gym's gamma = .5 / gamma = 0 networks
  P.arrive = ARR ? 1 : 0;
  P.max_steps = cf.steps;
  P.max_progress = __builtin_inf();
  P.max_time = __builtin_inf();
  P.policy = cf.policy < 4 ? cf.policy : 0;
  P.cap = cf.steps + 64 < 4096 ? cf.steps + 64 : 4096;  // release indices fit a list entry
  if (!lazy_clock_ok(P)) {
    fprintf(stderr, "lazy clock not applicable: delta %g steps %d\n", cf.delta, cf.steps);
    exit(2);
  }
  P.u_lazy = lazy_threshold(P);
  const uint64_t seed = 0x5eed0000ull;
  std::vector<uint4> rq(W * PER_LANE);
  std::vector<int32_t> flag(W, 0);
  std::vector<uint32_t> rep(2 * W);
  std::vector<std::vector<double>> ring(W, std::vector<double>(RING)),
      spill(W, std::vector<double>(P.cap));
  std::vector<std::vector<uint8_t>> replay(W, std::vector<uint8_t>(REPLAY_BYTES));
  std::vector<LaneMem> MF(W), ME(W);
  std::vector<ZStream> S(W);
  std::vector<NakLane> F(W), E(W);  // fast (as the timed kernels), eager (general)
  std::vector<int> bad(W, 0);
  for (int i = 0; i < W; ++i) {
    const uint64_t ep = ep0 + i;
    S[i].k0 = (uint32_t)seed;
    S[i].k1 = (uint32_t)(seed >> 32);
    S[i].e0 = (uint32_t)ep;
    S[i].e1 = (uint32_t)(ep >> 32);
    S[i].zero_at = i == 0 ? zero_lane0 : 0xffffffffu;
    MF[i].times = false;
    MF[i].d2 = D2;
    MF[i].cap = P.cap;
    MF[i].rq = rq.data();
    MF[i].rq_cap = W * PER_LANE;
    MF[i].rflag = flag.data();
    MF[i].rep = rep.data();
    MF[i].lane = i;
    MF[i].wave = W;
    ME[i].ring = ring[i].data();
    ME[i].spill = spill[i].data();
    ME[i].ring_stride = ME[i].spill_stride = 1;
    ME[i].cap = P.cap;
    ME[i].replay = ReplayMem::at(replay[i].data());
    F[i].init();
    E[i].init();
    F[i].template activate<ZStream, LZ>(P, S[i], MF[i]);
    E[i].activate(P, S[i], ME[i]);
    if (!view(F[i], P, MF[i]).same(view(E[i], P, ME[i]), !ARR)) bad[i] = 1;
  }
  auto drain = [&]() {
    for (int i = 0; i < W; ++i) races_publish(S[i], MF[i]);
    for (int i = 0; i < W; ++i) races_check<ZStream, LZ>(F[i], P, S[i], MF[i]);
    for (int i = 0; i < W; ++i) races_settle(F[i], MF[i]);
    ++C.drains;
  };
  std::vector<NakLane::Draw> df(W), de(W);
  for (int s = 0; s < cf.steps; ++s) {
    for (int i = 0; i < W; ++i) {
      df[i] = F[i].template draw<ZStream, LZ>(P, S[i]);
      de[i] = E[i].draw(P, S[i]);
      const int32_t m64 = miner64(S[i], (uint32_t)F[i].k, P.t_att, P.d);
      if (df[i].miner != m64 || de[i].miner != m64) ++C.miner_mismatches;
      C.alpha1_draws += cf.alpha >= 1.0 ? 1 : 0;
      const uint32_t uh = (uint32_t)(df[i].u >> 26);
      C.exact_entries += ((uh - 1u) >= (lazy_hi(P.u_lazy) - 1u) || F[i].tinf) ? 1 : 0;
      const int32_t act = cf.policy < 4 ? E[i].policy_action(P)
                                        : (int32_t)(mix(ep0 + i, s) & 3u);
      F[i].apply(act);
      E[i].apply(act);
      F[i].template resolve<ZStream, 0, TT>(P, S[i], MF[i]);
      E[i].template resolve<ZStream, 0, 0>(P, S[i], ME[i]);
    }
    if (ARR) {
      int32_t below = 0;  // enqueue_race: the racing lanes in lane order after the list
      for (int i = 0; i < W; ++i)
        if (F[i].rw) rq[F[i].qn + below++] = race_entry<LZ>(F[i], i);
      C.races += below;
      for (int i = 0; i < W; ++i) {
        F[i].qn += below;
        F[i].rw = 0u;
      }
    }
    for (int i = 0; i < W; ++i) {
      F[i].template activate<ZStream, LZ>(P, S[i], MF[i], df[i]);
      E[i].activate(P, S[i], ME[i], de[i]);
      if (!bad[i] && !view(F[i], P, MF[i]).same(view(E[i], P, ME[i]), !ARR)) {
        bad[i] = 1;
        if (!ARR)
          fprintf(stderr, "MISMATCH alpha=%g gamma=%g d=%d delta=%g pol=%d steps=%d ep=%llu step %d: "
                  "status fast %u eager %u\n", cf.alpha, cf.gamma, cf.d, cf.delta, cf.policy,
                  cf.steps, (unsigned long long)(ep0 + i), s, F[i].status, E[i].status);
      }
    }
    C.steps += W;
    if (ARR && races_due(F[0], MF[0])) drain();
  }
  if (ARR) drain();
  for (int i = 0; i < W; ++i) {
    ++C.episodes;
    C.overlaps += (E[i].status & ST_OVERLAP) ? 1 : 0;
    C.ties += (E[i].status & ST_TIE) ? 1 : 0;
    C.inf_eps += S[i].zero_at <= (uint32_t)cf.steps ? 1 : 0;
    if (F[i].status & ST_RACE_REDO) {  // the kernel discards this run
      ++C.redo;
      continue;
    }
    // (after the last verification the deferred lane's status is complete)
    if (ARR && !view(F[i], P, MF[i]).same(view(E[i], P, ME[i]), true)) bad[i] = 1;
    if (bad[i] && ARR)
      fprintf(stderr, "MISMATCH alpha=%g gamma=%g delta=%g pol=%d steps=%d ep=%llu: status fast %u "
              "eager %u\n", cf.alpha, cf.gamma, cf.delta, cf.policy, cf.steps,
              (unsigned long long)(ep0 + i), F[i].status, E[i].status);
    C.mismatches += bad[i];
  }
}

static void run_cfg(const Cfg& cf, int waves, Counters& C) {
  for (int w = 0; w < waves; ++w) {
    // every third wave draws a zero clock uniform (delay +inf) somewhere in its first lane
    const uint32_t z = w % 3 == 2 ? mix(w, cf.steps) % (uint32_t)cf.steps : 0xffffffffu;
    const uint64_t ep0 = 1000 + (uint64_t)W * w;
    if (cf.gamma > 0.0)
      run_wave<true, true>(cf, ep0, z, C);
    else if (cf.d == 2)
      run_wave<false, true>(cf, ep0, z, C);
    else
      run_wave<false, false>(cf, ep0, z, C);
  }
}

int main(int argc, char** argv) {
  const int n_short = argc > 1 ? atoi(argv[1]) : 24;
  const int n_long = argc > 2 ? atoi(argv[2]) : 4;
  Counters C;
  for (int steps : {300, 16384})
    for (double delta : {1e-9, 1e-5, 1e-3})
      for (int pol = 0; pol <= 4; ++pol) {
        if (pol == 1) continue;  // SM1, ES'14, honest and random actions
        const int waves = ((steps == 300 ? n_short : n_long) + W - 1) / W;
        for (double a : {0.05, 0.33, 0.45, 0.5}) {
          for (int d : {2, 3, 5}) run_cfg(Cfg{a, 0.0, delta, d, pol, steps}, waves, C);
          run_cfg(Cfg{a, 0.5, delta, 2, pol, steps}, waves, C);
        }
      }
  // alpha = 1: t_att = 2^32, every activation the attacker's
  for (int d : {2, 3}) run_cfg(Cfg{1.0, 0.0, 1e-5, d, 3, 300}, 2, C);
  run_cfg(Cfg{1.0, 0.5, 1e-5, 2, 3, 300}, 2, C);
  printf("{\"episodes\": %ld, \"steps\": %ld, \"mismatches\": %ld, \"miner_mismatches\": %ld, "
         "\"exact_branch_entries\": %ld, \"overlap_episodes\": %ld, \"tie_episodes\": %ld, "
         "\"redo_episodes\": %ld, \"inf_clock_episodes\": %ld, \"races\": %ld, \"drains\": %ld, "
         "\"alpha1_draws\": %ld}\n",
         C.episodes, C.steps, C.mismatches, C.miner_mismatches, C.exact_entries, C.overlaps,
         C.ties, C.redo, C.inf_eps, C.races, C.drains, C.alpha1_draws);
  return C.mismatches || C.miner_mismatches ? 1 : 0;
}
