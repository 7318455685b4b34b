// TEST INFRASTRUCTURE ONLY: cpr_amd/csrc/lane_env.h on the host, for tests/test_lane_env_host.py.
//   lane_env_host index SEED N_ALPHA N_EPISODES
//     prints lane_alpha_index(SEED, e, N_ALPHA) for e = 0 .. N_EPISODES - 1, one per line
//   lane_env_host wrap SCHEME SHAPE TARGET ALPHA FILE
//     FILE holds one step per line: "reset" (the lane's reset: the dense accumulator is
//     zeroed), or "reward done era erd progress n_activations" with the floats as C99 hex
//     floats; prints the wrapped and shaped reward of every step as 16 hex digits of its bits
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../cpr_amd/csrc/lane_env.h"

int main(int argc, char** argv) {
  if (argc == 5 && !strcmp(argv[1], "index")) {
    const uint64_t seed = strtoull(argv[2], nullptr, 10);
    const int32_t n_alpha = (int32_t)atoi(argv[3]);
    const long n_eps = atol(argv[4]);
    if (n_alpha < 1 || n_alpha > cpr::kLaneEnvMaxAlpha || n_eps < 0) return 2;
    for (long e = 0; e < n_eps; ++e)
      printf("%d\n", (int)cpr::lane_alpha_index(seed, (uint64_t)e, n_alpha));
    return 0;
  }
  if (argc == 7 && !strcmp(argv[1], "wrap")) {
    const int32_t scheme = (int32_t)atoi(argv[2]), shape = (int32_t)atoi(argv[3]);
    const double target = strtod(argv[4], nullptr), alpha = strtod(argv[5], nullptr);
    FILE* f = fopen(argv[6], "r");
    if (!f) return 2;
    std::vector<char> line(512);
    double acc = 0.0;
    while (fgets(line.data(), (int)line.size(), f)) {
      if (!strncmp(line.data(), "reset", 5)) {
        acc = 0.0;
        continue;
      }
      char* p = line.data();
      cpr::GymStepInfo s;
      s.reward = strtod(p, &p);
      s.done = strtol(p, &p, 10) != 0;
      s.era = strtod(p, &p);
      s.erd = strtod(p, &p);
      s.progress = strtod(p, &p);
      s.n_activations = strtoll(p, &p, 10);
      double r = cpr::gym_reward(scheme, target, s, &acc);
      r = cpr::shape_reward(shape, r, alpha, s);
      printf("%016llx\n", (unsigned long long)cpr::bitsd(r));
    }
    fclose(f);
    return 0;
  }
  fprintf(stderr, "usage: lane_env_host index SEED N_ALPHA N_EPISODES | wrap SCHEME SHAPE TARGET "
                  "ALPHA FILE\n");
  return 2;
}
