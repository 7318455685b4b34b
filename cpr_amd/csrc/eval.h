// The evaluation's per-alpha reduction (cpr_eval_net, DESIGN.md §4.14 "Evaluation"): what a
// cpr_eval_record contributes to a cpr_summary, and the order in which the f64 statistics are
// added up. Host-compilable, so that a native test pins both (tests/native_eval);
// k_eval_reduce (kernels_policy.hip) runs the same functions.
#pragma once
#include <math.h>
#include <stdint.h>

#include "../../include/cpr_hip.h"

#ifndef __host__
#define __host__
#define __device__
#endif

#pragma clang fp contract(off)

namespace cpr {

constexpr int kEvalThreads = 256;  // threads of a k_eval_reduce workgroup: the stride of p_t

// what summary.h's acc_episode takes of one finished episode
struct EvalTerms {
  int64_t ra_fx, rd_fx, prog_fx;  // 2^-20 fixed point
  double rel;                     // attacker share of the head's rewards, 0 if there are none
  int64_t height, steps, acts;
  uint32_t status;
};

// the fixed-point rule of every other summary (k_policy_collect) on a record
__host__ __device__ inline EvalTerms eval_terms(const cpr_eval_record& r) {
  EvalTerms t;
  const double ra = r.reward_attacker, rd = r.reward_defender;
  t.ra_fx = (int64_t)__builtin_rint(ra * 1048576.0);
  t.rd_fx = (int64_t)__builtin_rint(rd * 1048576.0);
  t.prog_fx = (int64_t)__builtin_rint(r.episode_progress * 1048576.0);
  t.rel = (ra + rd) != 0.0 ? ra / (ra + rd) : 0.0;
  t.height = r.height;
  t.steps = r.episode_n_steps;
  t.acts = r.episode_n_activations;
  t.status = r.status;
  return t;
}

// acc_episode (summary.h) on a cpr_summary in plain C++: the device adds the same integers
// through its workgroup reduction
__host__ __device__ inline void eval_summary_add(cpr_summary& s, const EvalTerms& t) {
  if (t.status & CPR_ST_INVALID) {
    s.steps += t.steps;
    s.activations += t.acts;
    s.invalid += 1;
    return;
  }
  s.episodes += 1;
  s.steps += t.steps;
  s.activations += t.acts;
  s.reward_attacker_fx += t.ra_fx;
  s.reward_defender_fx += t.rd_fx;
  s.progress_fx += t.prog_fx;
  s.orphans += t.acts - t.height;
  s.status_tie += (t.status & CPR_ST_TIE) ? 1 : 0;
  s.status_overlap += (t.status & CPR_ST_OVERLAP) ? 1 : 0;
  s.status_other +=
      (t.status & ~(uint32_t)(CPR_ST_TIE | CPR_ST_OVERLAP | CPR_ST_EXACT_RERUN)) ? 1 : 0;
  s.rel_revenue_fx += (uint64_t)__builtin_rint(t.rel * 4294967296.0);
  s.rel_revenue_sq_fx += (uint64_t)__builtin_rint(t.rel * t.rel * 4294967296.0);
  int bin = (int)(t.rel * (double)CPR_HIST_BINS);
  bin = bin < 0 ? 0 : (bin >= CPR_HIST_BINS ? CPR_HIST_BINS - 1 : bin);
  s.hist[bin] += 1;
}

__host__ __device__ inline bool eval_valid(const cpr_eval_record& r) {
  return (r.status & CPR_ST_INVALID) == 0;
}

// column c (enum cpr_eval_column) of a record: what EvalCallback logs
__host__ __device__ inline double eval_column(const cpr_eval_record& r, int c) {
  switch (c) {
    case CPR_EVAL_REWARD: return r.episode_reward;
    case CPR_EVAL_SIM_TIME: return r.episode_sim_time;
    case CPR_EVAL_CHAIN_TIME: return r.episode_chain_time;
    case CPR_EVAL_PROGRESS: return r.episode_progress;
    default: return (double)r.episode_n_activations;
  }
}

// An alpha's records: r_k = recs[k * stride], k < count. p_t of the documented order: thread t
// adds the valid records t, t + kEvalThreads, ... in that order, starting from 0; with
// centered, (x - mean)^2 in place of x.
__host__ __device__ inline double eval_partial(const cpr_eval_record* recs, int64_t stride,
                                               int64_t count, int t, int c, bool centered,
                                               double mean) {
  double p = 0.0;
  for (int64_t k = t; k < count; k += kEvalThreads) {
    const cpr_eval_record& r = recs[k * stride];
    if (!eval_valid(r)) continue;
    const double x = eval_column(r, c);
    if (centered) {
      const double d = x - mean;
      p = p + d * d;
    } else {
      p = p + x;
    }
  }
  return p;
}

// one level of the tree over p[0 .. kEvalThreads): thread t < off takes p[t + off]. Levels run
// off = kEvalThreads / 2, ..., 1, each after the one before has finished for every t.
__host__ __device__ inline void eval_tree_level(double* p, int t, int off) {
  if (t < off) p[t] = p[t] + p[t + off];
}

__host__ __device__ inline double eval_mean(double sum, int64_t n) {
  return n > 0 ? sum / (double)n : (double)NAN;
}
__host__ __device__ inline double eval_std(double ssd, int64_t n) {
  return n > 1 ? sqrt(ssd / (double)(n - 1)) : (double)NAN;
}

// The whole reduction of one alpha on the host, in the kernel's order (the native test).
inline void eval_reduce_host(const cpr_eval_record* recs, int64_t stride, int64_t count,
                             double alpha, cpr_summary* sum, cpr_eval_alpha* out) {
  int64_t n = 0;
  for (int64_t k = 0; k < count; ++k) {
    const cpr_eval_record& r = recs[k * stride];
    eval_summary_add(*sum, eval_terms(r));
    n += eval_valid(r) ? 1 : 0;
  }
  out->alpha = alpha;
  out->n = n;
  double p[kEvalThreads];
  for (int c = 0; c < CPR_EVAL_COLUMNS; ++c) {
    for (int pass = 0; pass < 2; ++pass) {
      for (int t = 0; t < kEvalThreads; ++t)
        p[t] = eval_partial(recs, stride, count, t, c, pass == 1, out->mean[c]);
      for (int off = kEvalThreads / 2; off > 0; off >>= 1)
        for (int t = 0; t < off; ++t) eval_tree_level(p, t, off);
      if (pass == 0)
        out->mean[c] = eval_mean(p[0], n);
      else
        out->std[c] = eval_std(p[0], n);
    }
  }
}

}  // namespace cpr
