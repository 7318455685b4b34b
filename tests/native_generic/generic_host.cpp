// TEST INFRASTRUCTURE ONLY: cpr_amd/csrc/generic_lane.h on the host, for
// tests/test_generic_env_host.py.
//   generic_host T_ALPHA T_GAMMA T_TERM MAX_STEPS SEED FILE
//     FILE holds one command per line: "reset EPISODE" (generic_start) or "step ACTION"
//     (generic_env_step with the integer action). Prints per command
//       a d mf n_release n_consider n_blocks rewrite reward progress terminated truncated
//       status o0 o1 o2 o3 o4
//     with the observation (generic_observe) as 8 hex digits of each float's bits; a reset
//     prints 0 for reward, progress, terminated and truncated.
//   generic_host codec
//     prints encode(a) bits and decode(encode(a)) for a = -256 .. 256, then reads floats as
//     8 hex digits from stdin and prints their decoding, or "raises".
//   With GARBAGE=<seed> the lane's header and block storage start out as pseudo-random bytes
//   (tests/native/garbage.h) before every reset.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../cpr_amd/csrc/generic_lane.h"
#include "../native/garbage.h"

using namespace cpr;
using namespace cpr::generic;

static uint32_t bitsf(float f) { return __builtin_bit_cast(uint32_t, f); }

static void print(const GenericBlocks& B, GenericLane& L, const GenericStep& t, bool done) {
  const GenericObs f = generic_observe_fields(B, L);
  float o[5];
  generic_observe(B, L, o);
  printf("%d %d %d %d %d %d %d %d %d %d %d %u %08x %08x %08x %08x %08x\n", f.a, f.d, f.mf,
         L.n_rel, L.n_con, L.n_blocks, L.last_rewrite, t.reward_attacker, t.progress,
         t.terminated ? 1 : 0, (done && !t.terminated) ? 1 : 0, L.status, bitsf(o[0]),
         bitsf(o[1]), bitsf(o[2]), bitsf(o[3]), bitsf(o[4]));
}

static int codec() {
  for (int a = -256; a <= 256; ++a) {
    const float e = generic_encode_action(a);
    int32_t d = 9999;
    const bool ok = generic_decode_action(e, &d);
    printf("%d %08x %d\n", a, bitsf(e), ok ? d : 9999);
  }
  char line[64];
  while (fgets(line, sizeof(line), stdin)) {
    const uint32_t u = (uint32_t)strtoul(line, nullptr, 16);
    int32_t d;
    if (generic_decode_action(__builtin_bit_cast(float, u), &d))
      printf("%d\n", d);
    else
      printf("raises\n");
  }
  return 0;
}

int main(int argc, char** argv) {
  if (argc == 2 && !strcmp(argv[1], "codec")) return codec();
  if (argc != 7) {
    fprintf(stderr, "usage: generic_host T_ALPHA T_GAMMA T_TERM MAX_STEPS SEED FILE\n");
    return 2;
  }
  GenericParams P;
  memset(&P, 0, sizeof(P));
  P.t_alpha = strtoull(argv[1], nullptr, 10);
  P.t_gamma = strtoull(argv[2], nullptr, 10);
  P.t_term = strtoull(argv[3], nullptr, 10);
  P.max_steps = atoi(argv[4]);
  if (P.max_steps <= 0 || P.max_steps > kGenericMaxSteps) return 2;
  const uint64_t seed = strtoull(argv[5], nullptr, 10);
  FILE* f = fopen(argv[6], "r");
  if (!f) return 2;
  // exactly the lane's region, so the sanitizer sees any access beyond it
  std::vector<uint8_t> mem(generic_region_bytes(P.max_steps));
  const GenericBlocks B = generic_blocks(mem.data(), P.max_steps);
  GenericLane L;
  memset(&L, 0, sizeof(L));
  std::vector<char> line(256);
  Stream S = {};
  while (fgets(line.data(), (int)line.size(), f)) {
    if (!strncmp(line.data(), "reset ", 6)) {
      const uint64_t ep = strtoull(line.data() + 6, nullptr, 10);
      S.k0 = (uint32_t)seed;
      S.k1 = (uint32_t)(seed >> 32);
      S.e0 = (uint32_t)ep;
      S.e1 = (uint32_t)(ep >> 32);
      fill_garbage(mem);
      fill_garbage(&L, sizeof(L));
      generic_start(B, L, ep);
      print(B, L, GenericStep{0, 0, 0, 0, 0, false}, false);
    } else if (!strncmp(line.data(), "step ", 5)) {
      if (L.live == 0) return 3;
      GenericStep t;
      const bool done = generic_env_step(P, S, B, L, (int32_t)atoi(line.data() + 5), &t,
                                         [](bool, bool) {});
      print(B, L, t, done);
    } else {
      return 2;
    }
  }
  fclose(f);
  return 0;
}
