// TEST INFRASTRUCTURE ONLY: cpr_amd/csrc/fc16_lane.h on the host, for
// tests/test_fc16_env_host.py.
//   fc16_host T_ALPHA T_GAMMA T_TERM SEED FILE
//     FILE holds one command per line: "reset EPISODE" (fc16_start) or "step INDEX"
//     (fc16_action_name, then fc16_step). Prints per command
//       a h fork reward progress terminated steps o0 o1 o2
//     with the observation (fc16_observe) as 16 hex digits of each double's bits; a reset
//     prints 0 for reward, progress and terminated.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../cpr_amd/csrc/fc16_lane.h"

using namespace cpr;

static void print(const fc16::Fc16State& s, int r, int g, int term) {
  double o[3];
  fc16::fc16_observe(s, o);
  printf("%d %d %d %d %d %d %lld %016llx %016llx %016llx\n", s.a, s.h, s.fork, r, g, term,
         (long long)s.steps, (unsigned long long)bitsd(o[0]), (unsigned long long)bitsd(o[1]),
         (unsigned long long)bitsd(o[2]));
}

int main(int argc, char** argv) {
  if (argc != 6) {
    fprintf(stderr, "usage: fc16_host T_ALPHA T_GAMMA T_TERM SEED FILE\n");
    return 2;
  }
  fc16::Fc16Params P;
  memset(&P, 0, sizeof(P));
  P.t_alpha = strtoull(argv[1], nullptr, 10);
  P.t_gamma = strtoull(argv[2], nullptr, 10);
  P.t_term = strtoull(argv[3], nullptr, 10);
  P.max_steps = (int64_t)1 << 30;
  const uint64_t seed = strtoull(argv[4], nullptr, 10);
  FILE* f = fopen(argv[5], "r");
  if (!f) return 2;
  std::vector<char> line(256);
  Stream S = {};
  fc16::Fc16State s = {};
  bool live = false;
  while (fgets(line.data(), (int)line.size(), f)) {
    if (!strncmp(line.data(), "reset ", 6)) {
      const uint64_t ep = strtoull(line.data() + 6, nullptr, 10);
      S.k0 = (uint32_t)seed;
      S.k1 = (uint32_t)(seed >> 32);
      S.e0 = (uint32_t)ep;
      S.e1 = (uint32_t)(ep >> 32);
      s = fc16::fc16_start(P, S);
      live = true;
      print(s, 0, 0, 0);
    } else if (!strncmp(line.data(), "step ", 5)) {
      if (!live) return 3;
      const int32_t index = (int32_t)atoi(line.data() + 5);
      const fc16::Fc16Step t = fc16::fc16_step(P, S, s, fc16::fc16_action_name(s.a, s.h, index));
      print(s, t.reward, t.progress, t.terminated ? 1 : 0);
    } else {
      return 2;
    }
  }
  fclose(f);
  return 0;
}
