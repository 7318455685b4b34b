// TEST INFRASTRUCTURE ONLY: cpr_amd/csrc/eval.h and lane_env.h's cyclic schedule on the host, for
// tests/test_eval_host.py.
//   eval_host cycle N_ALPHA FIRST COUNT
//     prints lane_alpha_entry(CPR_SCHEDULE_CYCLE, 0, e, N_ALPHA) for e = FIRST .. FIRST + COUNT - 1
//   eval_host reduce FILE N_ALPHA FIRST
//     FILE holds cpr_eval_record structs, record s being episode FIRST + s; for every table
//     entry j (its records: the slots s with (FIRST + s) mod N_ALPHA = j, in order) prints one
//     line: j, n, the 13 scalar words of its cpr_summary in struct order, the 64 histogram
//     bins, then mean and std of the five columns as 16 hex digits of their bits
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../cpr_amd/csrc/eval.h"
#include "../../cpr_amd/csrc/lane_env.h"

int main(int argc, char** argv) {
  if (argc == 5 && !strcmp(argv[1], "cycle")) {
    const int32_t n_alpha = (int32_t)atoi(argv[2]);
    const uint64_t first = strtoull(argv[3], nullptr, 10);
    const long count = atol(argv[4]);
    if (n_alpha < 1 || n_alpha > cpr::kLaneEnvMaxAlpha || count < 0) return 2;
    for (long i = 0; i < count; ++i)
      printf("%d\n", (int)cpr::lane_alpha_entry(CPR_SCHEDULE_CYCLE, 0, first + (uint64_t)i, n_alpha));
    return 0;
  }
  if (argc == 5 && !strcmp(argv[1], "reduce")) {
    const int32_t A = (int32_t)atoi(argv[3]);
    const uint64_t first = strtoull(argv[4], nullptr, 10);
    FILE* f = fopen(argv[2], "rb");
    if (!f || A < 1) return 2;
    std::vector<cpr_eval_record> recs;
    cpr_eval_record r;
    while (fread(&r, sizeof(r), 1, f) == 1) recs.push_back(r);
    fclose(f);
    if (recs.empty() || recs.size() % (size_t)A != 0) return 2;
    const int64_t per_alpha = (int64_t)(recs.size() / (size_t)A);
    for (int32_t j = 0; j < A; ++j) {
      const int64_t s0 = (int64_t)(((uint64_t)j + (uint64_t)A - first % (uint64_t)A) % (uint64_t)A);
      cpr_summary s;
      memset(&s, 0, sizeof(s));
      cpr_eval_alpha out;
      memset(&out, 0, sizeof(out));
      cpr::eval_reduce_host(recs.data() + s0, A, per_alpha, recs[(size_t)s0].alpha, &s, &out);
      printf("%d %lld", (int)j, (long long)out.n);
      const long long w[13] = {s.episodes, s.steps, s.activations, s.reward_attacker_fx,
                               s.reward_defender_fx, s.progress_fx, (long long)s.rel_revenue_fx,
                               (long long)s.rel_revenue_sq_fx, s.orphans, s.status_tie,
                               s.status_overlap, s.status_other, s.invalid};
      for (long long v : w) printf(" %lld", v);
      for (int i = 0; i < CPR_HIST_BINS; ++i) printf(" %lld", (long long)s.hist[i]);
      for (int c = 0; c < CPR_EVAL_COLUMNS; ++c) {
        unsigned long long m, d;
        memcpy(&m, &out.mean[c], 8);
        memcpy(&d, &out.std[c], 8);
        printf(" %016llx %016llx", m, d);
      }
      printf("\n");
    }
    return 0;
  }
  fprintf(stderr, "usage: eval_host cycle N_ALPHA FIRST COUNT | reduce FILE N_ALPHA FIRST\n");
  return 2;
}
