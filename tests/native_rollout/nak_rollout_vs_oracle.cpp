// TEST INFRASTRUCTURE ONLY. The closed-form rollout step of the lockstep lanes
// (cpr_amd/csrc/nak_rollout.h, compiled here for the host: policy, action log, step, done
// rule, reward, auto-reset at episode id + n_lanes) beside the CPU oracle's gym
// (oracle/src/des.cpp) on the same keyed stream: sequential oracle episodes i, i + n, ...
// per lane with the oracle's own policy. Observation fields before every step, reward, done
// and the logged action must agree. Prints one JSON line; exit code 1 on any mismatch.
// Build: tests/native_rollout/Makefile (hipcc; only host code is executed).
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <memory>
#include <vector>

#include "../../cpr_amd/csrc/nak_rollout.h"
#include "../../oracle/src/des.h"

using namespace cpr;

// host stand-in for a lockstep lane's memory (kernels.hip lock_mem) and its action log
struct HostLane {
  std::vector<double> ring, spill;
  std::vector<uint8_t> replay, alog;
  HostLane(const NakParams& P, int64_t alog_cap)
      : ring(RING, -1.0), spill(P.cap, -1.0), replay(REPLAY_BYTES, 0xa5), alog(alog_cap, 0xff) {}
  LaneMem mem() {
    LaneMem M;
    M.ring = ring.data();
    M.spill = spill.data();
    M.ring_stride = M.spill_stride = 1;
    M.cap = (int32_t)spill.size();
    M.replay = ReplayMem::at(replay.data());
    return M;
  }
};

struct Counters {
  long mismatches = 0, episodes = 0, steps = 0, flagged = 0;
};

static void run_config(int policy, double alpha, double gamma, int n_lanes, int T, int max_steps,
                       uint64_t seed, Counters& C) {
  const int defenders = 2;
  oracle::GymParams gp;
  gp.alpha = alpha;
  gp.gamma = gamma;
  gp.defenders = defenders;
  gp.max_steps = max_steps;
  gp.unit_obs = false;

  NakParams P{};  // as capi.hip's validation of the selfish-mining network
  P.t_att = oracle::alpha_threshold(alpha);
  P.d = defenders;
  P.ev = 1.0;
  P.delta = 1e-9;
  const double dd = defenders;
  P.dmax = (dd - 1.) / dd * 1e-9 / gamma;
  P.arrive = std::isfinite(P.dmax) ? 1 : 0;
  P.max_steps = max_steps;
  P.max_progress = __builtin_inf();
  P.max_time = __builtin_inf();
  P.policy = policy;
  P.cap = ((max_steps + 2 + 63) / 64) * 64;

  for (int i = 0; i < n_lanes; i++) {
    HostLane hm(P, max_steps);
    const LaneMem M = hm.mem();
    LockLane LL{};
    roll_reset(LL, P, seed, M, (uint64_t)i);
    uint64_t ep = (uint64_t)i;
    auto g = std::make_unique<oracle::GymNakamoto>(gp, 1, nullptr, seed, ep);
    double obs[4];
    g->reset(obs);
    bool bad = false;
    for (int t = 0; t < T && !bad; t++) {
      const oracle::NakObs o = g->observe_int();
      int32_t h, a, d, e;
      LL.L.observe(&h, &a, &d, &e);
      if (h != o.public_blocks || a != o.private_blocks || d != o.diff_blocks || e != o.event)
        bad = true;
      const int act = oracle::nak_policy(policy, o, nullptr);
      bool done = false;
      oracle::StepInfo info{};
      const double rew = g->step(act, obs, &done, &info);
      const int64_t s0 = LL.steps;
      const RollStep r = roll_step(LL, P, seed, M, hm.alog.data(), (int64_t)hm.alog.size());
      if (LL.L.status & kInexact) C.flagged++;
      if (r.action != act || hm.alog[(size_t)s0] != (uint8_t)act) bad = true;
      if (r.reward != rew || (r.done != 0) != done) bad = true;
      if (r.ra != info.episode_reward_attacker || r.head.h != info.head_height ||
          LL.steps != info.episode_n_steps || LL.L.k != info.episode_n_activations)
        bad = true;
      roll_keep(LL, P, seed, M, r, n_lanes);
      C.steps++;
      if (done) {
        C.episodes++;
        ep += (uint64_t)n_lanes;
        g = std::make_unique<oracle::GymNakamoto>(gp, 1, nullptr, seed, ep);
        g->reset(obs);
        if (LL.ep != ep || LL.steps != 0 || LL.last_ra != 0.0) bad = true;
      }
      if (bad) {
        C.mismatches++;
        fprintf(stderr, "MISMATCH policy=%d alpha=%g gamma=%g lane=%d step=%d\n", policy, alpha,
                gamma, i, t);
      }
    }
    // the last observation too (after a done: the new episode's first)
    const oracle::NakObs o = g->observe_int();
    int32_t h, a, d, e;
    LL.L.observe(&h, &a, &d, &e);
    if (!bad && (h != o.public_blocks || a != o.private_blocks || d != o.diff_blocks ||
                 e != o.event))
      C.mismatches++;
  }
}

int main(int argc, char** argv) {
  const int n_lanes = argc > 1 ? atoi(argv[1]) : 32;
  const int T = argc > 2 ? atoi(argv[2]) : 300;
  const int max_steps = argc > 3 ? atoi(argv[3]) : 70;
  Counters C;
  for (int policy = 0; policy < 4; policy++)
    for (double alpha : {0.25, 0.42})
      for (double gamma : {0.0, 0.5}) run_config(policy, alpha, gamma, n_lanes, T, max_steps, 0x5eed0000ull, C);
  printf("{\"mismatches\": %ld, \"episodes\": %ld, \"steps\": %ld, \"flagged_steps\": %ld}\n",
         C.mismatches, C.episodes, C.steps, C.flagged);
  return C.mismatches ? 1 : 0;
}
