// Device helpers of the Nakamoto lockstep kernels (cpr_reset / cpr_step in kernels.hip, the
// rollout in kernels_nak_rollout.hip): a lane's memory, its exact-engine slot, observations.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "kernels.h"

#pragma clang fp contract(off)

namespace cpr {

// nakamoto_ssz action (0 Adopt .. 3 Wait) -> the Nakamoto-mode Ethereum lane's action index
// (eth::lane_action's mapping)
__device__ inline int32_t nak_to_eth_action(int32_t a) {
  constexpr int32_t map[4] = {eth::A_ADOPT_DISCARD, eth::A_OVERRIDE, eth::A_MATCH, eth::A_WAIT};
  return map[a & 3] * 4;
}

__device__ inline LaneMem lock_mem(const NakParams& P, const LockBuffers& B, int64_t i, int64_t n) {
  LaneMem M;
  M.ring = B.ring + i;
  M.ring_stride = n;
  M.spill = B.spill + i * P.cap;  // per lane, contiguous, as the fused kernel's
  M.spill_stride = 1;
  M.cap = P.cap;
  M.replay = ReplayMem::at(B.replay + i * REPLAY_BYTES);
  return M;
}

__device__ inline void write_obs_fields(int32_t h, int32_t a, int32_t d, int32_t ev, int unit,
                                        const double* tab_nn, const double* tab_sg,
                                        int32_t tab_n, double* o) {
  if (unit) {
    // ssz_tools.ml:29-40; host-tabulated (libm) for |x| < tab_n
    o[0] = h < tab_n ? tab_nn[h] : 2.0 / 3.141592653589793 * atan((double)h / 1.0);
    o[1] = a < tab_n ? tab_nn[a] : 2.0 / 3.141592653589793 * atan((double)a / 1.0);
    o[2] = (d > -tab_n && d < tab_n) ? tab_sg[d + tab_n]
                                     : 0.5 + (1.0 / 3.141592653589793 * atan((double)d / 1.0));
    o[3] = (double)ev / 1.0;
  } else {
    o[0] = (double)h;
    o[1] = (double)a;
    o[2] = (double)d;
    o[3] = (double)ev;
  }
}

__device__ inline void write_obs(const NakLane& L, int unit, const double* tab_nn,
                                 const double* tab_sg, int32_t tab_n, double* o) {
  int32_t h, a, d, ev;
  L.observe(&h, &a, &d, &ev);
  write_obs_fields(h, a, d, ev, unit, tab_nn, tab_sg, tab_n, o);
}

// a lockstep lane's slot on the exact event engine (k_lock_exact)
__device__ inline eth::EthMem lock_exact_mem(const eth::EthParams& EP, const LockBuffers& B,
                                             int32_t slot) {
  return eth::eth_mem_at(B.emem + (int64_t)slot * B.elane_bytes, EP.cap_b, EP.cap_e, EP.n);
}

}  // namespace cpr
