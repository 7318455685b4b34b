// Value iteration over explicit MDPs that share one topology (kernels_mdp.hip):
// the reference's explicit_mdp.py:97-177 loop, one point (one probability array) per solve, all
// points of a call in one launch. f64, one rounding per operation, transitions accumulated in
// their order, the first best action kept: the results equal cpr_amd.mdp.value_iteration bit
// for bit.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>

namespace cpr {

constexpr int kMdpThreads = 1024;  // resident path: threads of the one workgroup per point
constexpr int kMdpPer = 10;        // ... and the states a thread may own (new values in VGPRs)
constexpr int kMdpBlock = 256;     // global path: states per workgroup
// sweeps one launch of the resident kernel runs at most; the points' state waits in global
// memory between launches
constexpr int kMdpSweepsPerLaunch = 1024;
// global path: sweeps (launches) between two reads of the points' status by the host. A sweep of
// a stopped point costs one skipped workgroup per 256 states, so a late read wastes little; an
// early one stalls the queue for a copy. 64 sweeps are a few hundred microseconds of launches
constexpr int kMdpReadbackEvery = 64;
// sweeps a point may take when max_iter == 0; a point that reaches it is `not converged`
constexpr int64_t kMdpSweepCap = 1 << 20;

// The automatic path, from profiles/mdp_vi_speed.json (SSZ'16 model, 16 transition slots per
// state): a resident sweep streams a point's slots through one CU, 0.5 us per 1,000 slots, and
// points beyond one per CU queue up; a global sweep costs a launch, 7.4 us, and past that about
// 1 us per 560,000 slots over all points. Resident is chosen when it fits and its estimate is
// the lower one.
inline bool mdp_auto_resident(int64_t slots_per_point, int64_t P, int cus) {
  const int64_t c = cus > 0 ? cus : 1;
  const double resident_us = 0.5e-3 * (double)slots_per_point * (double)((P + c - 1) / c);
  const double global_us = 7.4 + (double)P * (double)slots_per_point / 560000.0;
  return resident_us <= global_us;
}

constexpr int32_t kMdpRunning = -1;  // device-side status of a point that has not stopped

// The dense padded form, state index fastest: slot (a, t) of state s at (a * T + t) * S + s.
// dst < 0 marks an unused slot (used = 0 on the host side); prb holds P such arrays.
struct MdpDev {
  int32_t S, A, T, P;
  const int32_t* dst;    // [A][T][S]
  const uint8_t* valid;  // [A][S]
  const double* rew;     // [A][T][S]
  const double* prg;     // [A][T][S]
  const double* prb;     // [P][A][T][S]
};

struct MdpRun {
  double stop_delta, discount;
  int64_t max_iter;  // > 0: the point stops after that sweep
  int64_t cap;       // max_iter == 0: the point stops `not converged` after that sweep
  // the resident path keeps a point's vectors in buffer 0; the global path reads buffer
  // (k - 1) & 1 and writes buffer k & 1 in sweep k, so a point that stopped after sweep i has
  // its result in buffer i & 1
  double* value[2];     // [P][S]
  double* progress[2];  // [P][S]
  int32_t* policy;      // [P][S]
  int32_t* status;      // [P] kMdpRunning, then a cpr_mdp_vi_status
  int64_t* iter;        // [P] sweeps done
  double* delta;        // [P] the last sweep's delta
  // global path: max |new - old| of sweeps k, k - 1, k + 1 as bit patterns, slot k % 3
  unsigned long long* acc;  // [P][3]
};

// whether one workgroup holds value and progress of S states (LDS and registers)
bool mdp_resident_fits(int64_t S);
// at most kMdpSweepsPerLaunch sweeps of every point that has not stopped
hipError_t launch_mdp_resident(const MdpDev& M, const MdpRun& R, hipStream_t st);
// sweep k (1-based) of every point whose sweep k - 1 did not stop it; records the stop of
// sweep k - 1 otherwise
hipError_t launch_mdp_sweep(const MdpDev& M, const MdpRun& R, int64_t k, hipStream_t st);

// ---- policy evaluation (explicit_mdp.py:328-378): E evaluations over one MdpDev, each with its
// own policy at one of the P points. The sweep bounds, the read-back interval and the sweep cap
// are value iteration's.

// resident path: a thread whose states are at most kMdpPeKeepPer and whose actions have at most
// kMdpPeKeepT transition slots keeps its slots in registers across the sweeps (56 VGPRs); the
// other shapes read them again in every sweep, coalesced along s
constexpr int kMdpPeKeepPer = 2;
constexpr int kMdpPeKeepT = 4;

// The automatic path, fitted to profiles/mdp_pe_speed.json (MI355X, 256 CUs; SSZ'16 model, T = 4
// slots per state and sweep; kernel time over the sweeps of the longest evaluation):
//   slots per evaluation          3,968 (992 states)   15,928 (3,982 states)
//   resident, 1 evaluation        1.95 us (kept)       10.2 us (re-read)
//   resident re-read, 1           3.76 us              10.2 us
//   global, 1                     4.93 us              6.38 us   (5.34 and 5.39 in another run)
//   resident, 783 evaluations     5.2 us               19.1 us
//   global, 783                   10.6 us              25.4 us
// A resident sweep of one evaluation is 1.6 us (two barriers, the reduction) and 0.54 us per
// 1,000 slots read again, the line through the two re-read figures; slots kept in registers
// cost 0.09 us per 1,000, from the one kept shape measured with the same 1.6 us. Evaluations
// beyond one per CU queue up, but they stop at different sweeps and a free CU takes the next
// one: 783 evaluations on 256 CUs (3.06 per CU) cost 2.7 and 1.9 times a single one's sweep,
// 0.88 and 0.61 of 3.06; the rule takes 0.75. A global sweep is a launch, 5.3 us, and then
// 1 us per 600,000 slots over all evaluations (585,000 and 620,000 measured). With these the
// rule took the faster path at all four shapes of the profile.
inline bool mdp_pe_auto_resident(int64_t slots_per_eval, int64_t E, int cus, bool keep) {
  const double c = cus > 0 ? (double)cus : 1.0;
  const double one = 1.6 + (keep ? 0.09e-3 : 0.54e-3) * (double)slots_per_eval;
  const double resident_us = one * std::max(1.0, 0.75 * (double)E / c);
  const double global_us = 5.3 + (double)E * (double)slots_per_eval / 600000.0;
  return resident_us <= global_us;
}

struct MdpPeRun {
  double theta, discount;
  int64_t max_iter;  // > 0: the evaluation stops after that sweep
  int64_t cap;       // max_iter == 0: the evaluation stops `not converged` after that sweep
  int32_t E;
  int32_t reread;        // resident path: never keep the slots in registers (a measurement hook)
  const int32_t* point;  // [E]
  // [E][S] the action slot an included state plays, -1 for a state that stays 0 (not included,
  // or without a policy entry): the host's reachability walk folded into the policy
  const int32_t* act;
  // buffers as MdpRun's value / progress: resident in buffer 0, global in buffer iter & 1
  double* reward[2];    // [E][S]
  double* progress[2];  // [E][S]
  int32_t* status;      // [E] kMdpRunning, then a cpr_mdp_pe_status
  int64_t* iter;        // [E]
  double* delta;        // [E]
  unsigned long long* acc;  // [E][3] as MdpRun's
};

bool mdp_pe_resident_fits(int64_t S);
// whether the resident launch of this shape keeps the slots in registers
bool mdp_pe_resident_keeps(int64_t S, int32_t T);
hipError_t launch_mdp_pe_resident(const MdpDev& M, const MdpPeRun& R, hipStream_t st);
hipError_t launch_mdp_pe_sweep(const MdpDev& M, const MdpPeRun& R, int64_t k, hipStream_t st);

}  // namespace cpr
