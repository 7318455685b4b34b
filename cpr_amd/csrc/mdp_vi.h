// Value iteration over explicit MDPs that share one topology (kernels_mdp.hip):
// the reference's explicit_mdp.py:97-177 loop, one point (one probability array) per solve, all
// points of a call in one launch. f64, one rounding per operation, transitions accumulated in
// their order, the first best action kept: the results equal cpr_amd.mdp.value_iteration bit
// for bit.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

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

}  // namespace cpr
