// gfx950 kernels of value iteration over explicit MDPs (mdp_vi.h):
//   k_mdp_vi_resident  one workgroup per point; value and progress of every state in dynamic
//                      LDS, a thread's new values in registers across the barrier, the sweep's
//                      delta reduced in the workgroup, at most kMdpSweepsPerLaunch sweeps
//   k_mdp_vi_sweep     one sweep of every running point over points x states; value and
//                      progress ping-pong in global memory, delta by atomicMax on the bit
//                      pattern, the stop of the previous sweep decided by every workgroup alike
// and of policy evaluation over them (k_mdp_pe_resident, k_mdp_pe_sweep: the same two shapes
// for E evaluations, each a fixed policy at one point; below).
// Workgroups never wait for one another inside a kernel. No FMA: one rounding per operation.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "../../include/cpr_hip.h"
#include "kernels.h"
#include "mdp_vi.h"

#pragma clang fp contract(off)

namespace cpr {

// explicit_mdp.py:116-146 for one state: per valid action the used transitions accumulate in
// their order; an action is taken when `this_v > best_v or best_a < 0`.
// A sweep is bound by the latency of its loads, not by their bytes, so nothing here branches on
// loaded data: the slots of an action are loaded kMdpChunk at a time before any is used (unused
// slots hold dst -1 and zeros; a slot index past T - 1 reads slot T - 1 again), an unused slot
// or an invalid action is computed and then not selected, as the host's np.where does.
constexpr int kMdpChunk = 4;
__device__ __forceinline__ void mdp_state(const MdpDev& M, const double* prb, int64_t s,
                                          double discount, const double* v_prev,
                                          const double* p_prev, double& best_v, double& best_p,
                                          int32_t& best_a) {
  const int64_t S = M.S;
  const int32_t T = M.T;
  best_a = -1;
  best_v = 0.0;
  best_p = 0.0;
#pragma unroll 2
  for (int32_t a = 0; a < M.A; ++a) {
    const bool ok = M.valid[a * S + s] != 0;
    double this_v = 0.0, this_p = 0.0;
    for (int32_t t0 = 0; t0 < T; t0 += kMdpChunk) {
      int32_t d[kMdpChunk];
      double pr[kMdpChunk], rw[kMdpChunk], pg[kMdpChunk], vv[kMdpChunk], pp[kMdpChunk];
#pragma unroll
      for (int j = 0; j < kMdpChunk; ++j) {
        const int32_t t = t0 + j < T ? t0 + j : T - 1;
        const int64_t slot = ((int64_t)a * T + t) * S + s;
        d[j] = M.dst[slot];
        pr[j] = prb[slot];
        rw[j] = M.rew[slot];
        pg[j] = M.prg[slot];
      }
#pragma unroll
      for (int j = 0; j < kMdpChunk; ++j) {
        const int32_t from = d[j] < 0 ? 0 : d[j];
        vv[j] = v_prev[from];
        pp[j] = p_prev[from];
      }
#pragma unroll
      for (int j = 0; j < kMdpChunk; ++j) {
        const bool used = t0 + j < T && d[j] >= 0;
        const double tv = pr[j] * (rw[j] + discount * vv[j]);
        const double tp = pr[j] * (pg[j] + discount * pp[j]);
        this_v = used ? this_v + tv : this_v;
        this_p = used ? this_p + tp : this_p;
      }
    }
    const bool take = ok && (this_v > best_v || best_a < 0);
    best_a = take ? a : best_a;
    best_v = take ? this_v : best_v;
    best_p = take ? this_p : best_p;
  }
}

// the stop decision after sweep `it` with that sweep's delta: kMdpRunning or the final status
__device__ __forceinline__ int32_t mdp_stop(const MdpRun& R, int64_t it, double delta) {
  if (R.max_iter > 0 && it >= R.max_iter) return CPR_MDP_VI_MAX_ITER;
  if (delta <= R.stop_delta) return CPR_MDP_VI_CONVERGED;
  if (R.max_iter == 0 && it >= R.cap) return CPR_MDP_VI_NOT_CONVERGED;
  return kMdpRunning;
}

// |x| of a double orders like its bit pattern (a NaN above every number, so that a NaN delta
// never meets stop_delta)
__device__ __forceinline__ unsigned long long mdp_abs_bits(double x) {
  return (unsigned long long)__double_as_longlong(fabs(x));
}

__device__ __forceinline__ unsigned long long mdp_wave_max(unsigned long long v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const unsigned long long w = __shfl_xor(v, o, 64);
    v = w > v ? w : v;
  }
  return v;
}

extern __shared__ __attribute__((aligned(16))) unsigned char mdp_lds[];

// dynamic LDS: value[S], progress[S], one delta word per wave
static size_t mdp_resident_lds(int64_t S) {
  return (size_t)S * 16 + (kMdpThreads / 64) * 8;
}

// PER: the states a thread owns at most (its new values stay in registers across the barrier)
template <int PER>
__global__ __launch_bounds__(kMdpThreads) void k_mdp_vi_resident(MdpDev M, MdpRun R) {
  const int32_t p = blockIdx.x;
  if (R.status[p] != kMdpRunning) return;  // uniform: written only at the end of a launch
  const int32_t S = M.S, nt = blockDim.x, tid = threadIdx.x;
  double* lv = (double*)mdp_lds;
  double* lp = lv + S;
  unsigned long long* red = (unsigned long long*)(lp + S);
  double* gv = R.value[0] + (int64_t)p * S;
  double* gp = R.progress[0] + (int64_t)p * S;
  const double* prb = M.prb + (int64_t)p * M.A * M.T * S;
  for (int32_t s = tid; s < S; s += nt) {
    lv[s] = gv[s];
    lp[s] = gp[s];
  }
  int64_t it = R.iter[p];
  __syncthreads();
  double nv[PER], np[PER];
  int32_t na[PER];
  int32_t st = kMdpRunning;
  double delta = 0.0;
  for (int n = 0; n < kMdpSweepsPerLaunch; ++n) {
    unsigned long long dmax = 0;
#pragma unroll
    for (int k = 0; k < PER; ++k) {
      const int32_t s = tid + k * nt;
      if (s < S) {
        mdp_state(M, prb, s, R.discount, lv, lp, nv[k], np[k], na[k]);
        dmax = std::max(dmax, mdp_abs_bits(nv[k] - lv[s]));
      }
    }
    dmax = mdp_wave_max(dmax);
    if ((tid & 63) == 0) red[tid >> 6] = dmax;
    __syncthreads();  // every read of the previous vectors is done
    dmax = 0;
    for (int w = 0; w < nt / 64; ++w) dmax = std::max(dmax, red[w]);
#pragma unroll
    for (int k = 0; k < PER; ++k) {
      const int32_t s = tid + k * nt;
      if (s < S) {
        lv[s] = nv[k];
        lp[s] = np[k];
      }
    }
    ++it;
    delta = __longlong_as_double((long long)dmax);
    st = mdp_stop(R, it, delta);  // uniform: every thread holds the same delta
    __syncthreads();
    if (st != kMdpRunning) break;
  }
#pragma unroll
  for (int k = 0; k < PER; ++k) {
    const int32_t s = tid + k * nt;
    if (s < S) {
      gv[s] = nv[k];
      gp[s] = np[k];
      R.policy[(int64_t)p * S + s] = na[k];
    }
  }
  if (tid == 0) {
    R.iter[p] = it;
    R.delta[p] = delta;
    R.status[p] = st;
  }
}

__global__ __launch_bounds__(kMdpBlock) void k_mdp_vi_sweep(MdpDev M, MdpRun R, int64_t k,
                                                            int32_t chunks) {
  const int32_t p = blockIdx.x / chunks, c = blockIdx.x % chunks;
  const int32_t tid = threadIdx.x;
  // a stop is written by workgroups that return before they compute, and every workgroup of
  // the point decides it alike below, so it does not matter which value a racing read sees
  if (R.status[p] != kMdpRunning) return;
  unsigned long long* acc = R.acc + (int64_t)p * 3;
  if (k > 1) {
    const double d_prev = __longlong_as_double((long long)acc[(k - 1) % 3]);
    const int32_t st = mdp_stop(R, k - 1, d_prev);
    if (st != kMdpRunning) {
      if (c == 0 && tid == 0) {
        R.iter[p] = k - 1;
        R.delta[p] = d_prev;
        R.status[p] = st;
      }
      return;
    }
  }
  // the next sweep's slot: last read in launch k - 1, next written in launch k + 1
  if (c == 0 && tid == 0) acc[(k + 1) % 3] = 0;
  const int32_t S = M.S;
  const int32_t s = c * kMdpBlock + tid;
  unsigned long long dmax = 0;
  if (s < S) {
    const int in = (int)((k - 1) & 1), out = (int)(k & 1);
    const int64_t base = (int64_t)p * S;
    const double* v_prev = R.value[in] + base;
    double bv, bp;
    int32_t ba;
    mdp_state(M, M.prb + (int64_t)p * M.A * M.T * S, s, R.discount, v_prev,
              R.progress[in] + base, bv, bp, ba);
    R.value[out][base + s] = bv;
    R.progress[out][base + s] = bp;
    R.policy[base + s] = ba;
    dmax = mdp_abs_bits(bv - v_prev[s]);
  }
  dmax = mdp_wave_max(dmax);
  if ((tid & 63) == 0 && dmax) atomicMax(&acc[k % 3], dmax);
}

// ---------------------------------------------------------------- launchers

static int64_t mdp_lds_limit() {
  return std::min<int64_t>(lds_dynamic_max((const void*)k_mdp_vi_resident<kMdpPer>),
                           160 * 1024 - 2048);
}

bool mdp_resident_fits(int64_t S) {
  return S >= 1 && S <= (int64_t)kMdpThreads * kMdpPer &&
         (int64_t)mdp_resident_lds(S) <= mdp_lds_limit();
}

template <int PER>
static hipError_t launch_mdp_resident_per(const MdpDev& M, const MdpRun& R, int threads,
                                          int64_t bytes, hipStream_t st) {
  CPR_LDS_GUARD(k_mdp_vi_resident<PER>, bytes);
  if (bytes > 64 * 1024) {
    const hipError_t e = hipFuncSetAttribute(
        (const void*)k_mdp_vi_resident<PER>, hipFuncAttributeMaxDynamicSharedMemorySize,
        (int)std::min<int64_t>(lds_dynamic_max((const void*)k_mdp_vi_resident<PER>),
                               160 * 1024 - 2048));
    if (e != hipSuccess) return e;
  }
  hipLaunchKernelGGL(k_mdp_vi_resident<PER>, dim3((unsigned)M.P), dim3(threads), (size_t)bytes,
                     st, M, R);
  return hipGetLastError();
}

hipError_t launch_mdp_resident(const MdpDev& M, const MdpRun& R, hipStream_t st) {
  if (!mdp_resident_fits(M.S)) return hipErrorInvalidValue;
  const int64_t bytes = (int64_t)mdp_resident_lds(M.S);
  // whole waves; a thread owns the states tid, tid + threads, ... (the instantiation with the
  // fewest register-held states that covers them: fewer live registers, no scratch)
  const int threads = (int)std::min<int64_t>(kMdpThreads, (M.S + 63) / 64 * 64);
  const int64_t per = (M.S + threads - 1) / threads;
  if (per <= 1) return launch_mdp_resident_per<1>(M, R, threads, bytes, st);
  if (per <= 2) return launch_mdp_resident_per<2>(M, R, threads, bytes, st);
  if (per <= 4) return launch_mdp_resident_per<4>(M, R, threads, bytes, st);
  if (per <= kMdpPer) return launch_mdp_resident_per<kMdpPer>(M, R, threads, bytes, st);
  return hipErrorInvalidValue;
}

hipError_t launch_mdp_sweep(const MdpDev& M, const MdpRun& R, int64_t k, hipStream_t st) {
  const int64_t chunks = ((int64_t)M.S + kMdpBlock - 1) / kMdpBlock;
  if (k < 1 || chunks * M.P > INT32_MAX) return hipErrorInvalidValue;
  hipLaunchKernelGGL(k_mdp_vi_sweep, dim3((unsigned)(chunks * M.P)), dim3(kMdpBlock), 0, st, M, R,
                     k, (int32_t)chunks);
  return hipGetLastError();
}

// ---------------------------------------------------------------- policy evaluation
//   k_mdp_pe_resident  one workgroup per evaluation; reward and progress of every state in
//                      dynamic LDS as above. The policy is fixed, so a thread reads the same
//                      T slots of each of its states in every sweep: with KEEP it loads them
//                      once, before the first sweep, and a sweep touches LDS only
//   k_mdp_pe_sweep     one sweep of every running evaluation over evaluations x states
// explicit_mdp.py:350-366 for one state is one action's slots accumulated in their order.

// kMdpChunk slots of action `a` of state `s` from slot t0 on; a slot past T - 1 is unused
__device__ __forceinline__ void mdp_pe_load(const MdpDev& M, const double* prb, int64_t s,
                                            int32_t a, int32_t t0, int32_t (&d)[kMdpChunk],
                                            double (&pr)[kMdpChunk], double (&rw)[kMdpChunk],
                                            double (&pg)[kMdpChunk]) {
  const int64_t S = M.S;
  const int32_t T = M.T;
#pragma unroll
  for (int j = 0; j < kMdpChunk; ++j) {
    const bool in = t0 + j < T;
    const int64_t slot = ((int64_t)a * T + (in ? t0 + j : T - 1)) * S + s;
    const int32_t dj = M.dst[slot];
    d[j] = in ? dj : -1;
    pr[j] = prb[slot];
    rw[j] = M.rew[slot];
    pg[j] = M.prg[slot];
  }
}

// r += prb * (rew + discount * r_prev[dst]) and p likewise over the used slots of a chunk, in
// slot order; an unused slot (dst < 0) is computed and then not selected, as in mdp_state
__device__ __forceinline__ void mdp_pe_chunk(const int32_t (&d)[kMdpChunk],
                                             const double (&pr)[kMdpChunk],
                                             const double (&rw)[kMdpChunk],
                                             const double (&pg)[kMdpChunk], double discount,
                                             const double* r_prev, const double* p_prev,
                                             double& r, double& p) {
  double vv[kMdpChunk], pp[kMdpChunk];
#pragma unroll
  for (int j = 0; j < kMdpChunk; ++j) {
    const int32_t from = d[j] < 0 ? 0 : d[j];
    vv[j] = r_prev[from];
    pp[j] = p_prev[from];
  }
#pragma unroll
  for (int j = 0; j < kMdpChunk; ++j) {
    const double tr = pr[j] * (rw[j] + discount * vv[j]);
    const double tp = pr[j] * (pg[j] + discount * pp[j]);
    r = d[j] >= 0 ? r + tr : r;
    p = d[j] >= 0 ? p + tp : p;
  }
}

// state s playing slot a >= 0, its slots read from global memory
__device__ __forceinline__ void mdp_pe_state(const MdpDev& M, const double* prb, int64_t s,
                                             int32_t a, double discount, const double* r_prev,
                                             const double* p_prev, double& r, double& p) {
  r = 0.0;
  p = 0.0;
  for (int32_t t0 = 0; t0 < M.T; t0 += kMdpChunk) {
    int32_t d[kMdpChunk];
    double pr[kMdpChunk], rw[kMdpChunk], pg[kMdpChunk];
    mdp_pe_load(M, prb, s, a, t0, d, pr, rw, pg);
    mdp_pe_chunk(d, pr, rw, pg, discount, r_prev, p_prev, r, p);
  }
}

// explicit_mdp.py:368-376: `delta < theta` is strict and is asked before max_iter
__device__ __forceinline__ int32_t mdp_pe_stop(const MdpPeRun& R, int64_t it, double delta) {
  if (delta < R.theta) return CPR_MDP_PE_CONVERGED;
  if (R.max_iter > 0 && it >= R.max_iter) return CPR_MDP_PE_MAX_ITER;
  if (R.max_iter == 0 && it >= R.cap) return CPR_MDP_PE_NOT_CONVERGED;
  return kMdpRunning;
}

// PER as in k_mdp_vi_resident. KEEP (T <= kMdpChunk): a thread's slots live in registers
template <int PER, bool KEEP>
__global__ __launch_bounds__(kMdpThreads) void k_mdp_pe_resident(MdpDev M, MdpPeRun R) {
  static_assert(kMdpPeKeepT == kMdpChunk, "the kept slots are one chunk");
  const int32_t e = blockIdx.x;
  if (R.status[e] != kMdpRunning) return;  // uniform: written only at the end of a launch
  const int32_t S = M.S, nt = blockDim.x, tid = threadIdx.x;
  double* lr = (double*)mdp_lds;
  double* lp = lr + S;
  unsigned long long* red = (unsigned long long*)(lp + S);
  double* gr = R.reward[0] + (int64_t)e * S;
  double* gp = R.progress[0] + (int64_t)e * S;
  const double* prb = M.prb + (int64_t)R.point[e] * M.A * M.T * S;
  const int32_t* act = R.act + (int64_t)e * S;
  for (int32_t s = tid; s < S; s += nt) {
    lr[s] = gr[s];
    lp[s] = gp[s];
  }
  int32_t a[PER];
  constexpr int KP = KEEP ? PER : 1;
  int32_t kd[KP][kMdpChunk];
  double kpr[KP][kMdpChunk], krw[KP][kMdpChunk], kpg[KP][kMdpChunk];
#pragma unroll
  for (int k = 0; k < PER; ++k) {
    const int32_t s = tid + k * nt;
    a[k] = s < S ? act[s] : -1;
    if constexpr (KEEP) {
      // a state that stays 0 has no used slot
      mdp_pe_load(M, prb, s < S ? s : 0, a[k] < 0 ? 0 : a[k], 0, kd[k], kpr[k], krw[k], kpg[k]);
#pragma unroll
      for (int j = 0; j < kMdpChunk; ++j) kd[k][j] = a[k] < 0 ? -1 : kd[k][j];
    }
  }
  int64_t it = R.iter[e];
  __syncthreads();
  double nr[PER], np[PER];
  int32_t st = kMdpRunning;
  double delta = 0.0;
  for (int n = 0; n < kMdpSweepsPerLaunch; ++n) {
    unsigned long long dmax = 0;
#pragma unroll
    for (int k = 0; k < PER; ++k) {
      const int32_t s = tid + k * nt;
      if (s < S) {
        nr[k] = 0.0;
        np[k] = 0.0;
        if constexpr (KEEP) {
          mdp_pe_chunk(kd[k], kpr[k], krw[k], kpg[k], R.discount, lr, lp, nr[k], np[k]);
        } else {
          if (a[k] >= 0) mdp_pe_state(M, prb, s, a[k], R.discount, lr, lp, nr[k], np[k]);
        }
        dmax = std::max(dmax, mdp_abs_bits(nr[k] - lr[s]));
      }
    }
    dmax = mdp_wave_max(dmax);
    if ((tid & 63) == 0) red[tid >> 6] = dmax;
    __syncthreads();  // every read of the previous vectors is done
    dmax = 0;
    for (int w = 0; w < nt / 64; ++w) dmax = std::max(dmax, red[w]);
#pragma unroll
    for (int k = 0; k < PER; ++k) {
      const int32_t s = tid + k * nt;
      if (s < S) {
        lr[s] = nr[k];
        lp[s] = np[k];
      }
    }
    ++it;
    delta = __longlong_as_double((long long)dmax);
    st = mdp_pe_stop(R, it, delta);  // uniform: every thread holds the same delta
    __syncthreads();
    if (st != kMdpRunning) break;
  }
#pragma unroll
  for (int k = 0; k < PER; ++k) {
    const int32_t s = tid + k * nt;
    if (s < S) {
      gr[s] = nr[k];
      gp[s] = np[k];
    }
  }
  if (tid == 0) {
    R.iter[e] = it;
    R.delta[e] = delta;
    R.status[e] = st;
  }
}

__global__ __launch_bounds__(kMdpBlock) void k_mdp_pe_sweep(MdpDev M, MdpPeRun R, int64_t k,
                                                            int32_t chunks) {
  const int32_t e = blockIdx.x / chunks, c = blockIdx.x % chunks;
  const int32_t tid = threadIdx.x;
  // as in k_mdp_vi_sweep: every workgroup of the evaluation decides the stop alike
  if (R.status[e] != kMdpRunning) return;
  unsigned long long* acc = R.acc + (int64_t)e * 3;
  if (k > 1) {
    const double d_prev = __longlong_as_double((long long)acc[(k - 1) % 3]);
    const int32_t st = mdp_pe_stop(R, k - 1, d_prev);
    if (st != kMdpRunning) {
      if (c == 0 && tid == 0) {
        R.iter[e] = k - 1;
        R.delta[e] = d_prev;
        R.status[e] = st;
      }
      return;
    }
  }
  if (c == 0 && tid == 0) acc[(k + 1) % 3] = 0;
  const int32_t S = M.S;
  const int32_t s = c * kMdpBlock + tid;
  unsigned long long dmax = 0;
  if (s < S) {
    const int64_t base = (int64_t)e * S;
    // a state that stays 0 is never written: both buffers hold 0 from the start
    const int32_t a = R.act[base + s];
    if (a >= 0) {
      const int in = (int)((k - 1) & 1), out = (int)(k & 1);
      const double* r_prev = R.reward[in] + base;
      double r, p;
      mdp_pe_state(M, M.prb + (int64_t)R.point[e] * M.A * M.T * S, s, a, R.discount, r_prev,
                   R.progress[in] + base, r, p);
      R.reward[out][base + s] = r;
      R.progress[out][base + s] = p;
      dmax = mdp_abs_bits(r - r_prev[s]);
    }
  }
  dmax = mdp_wave_max(dmax);
  if ((tid & 63) == 0 && dmax) atomicMax(&acc[k % 3], dmax);
}

// no instantiation has static LDS, so one answers for all; every launch is guarded on its own
static int64_t mdp_pe_lds_limit() {
  return std::min<int64_t>(lds_dynamic_max((const void*)k_mdp_pe_resident<kMdpPer, false>),
                           160 * 1024 - 2048);
}

bool mdp_pe_resident_fits(int64_t S) {
  return S >= 1 && S <= (int64_t)kMdpThreads * kMdpPer &&
         (int64_t)mdp_resident_lds(S) <= mdp_pe_lds_limit();
}

bool mdp_pe_resident_keeps(int64_t S, int32_t T) {
  return T <= kMdpPeKeepT && S <= (int64_t)kMdpThreads * kMdpPeKeepPer;
}

template <int PER, bool KEEP>
static hipError_t launch_mdp_pe_resident_per(const MdpDev& M, const MdpPeRun& R, int threads,
                                             int64_t bytes, hipStream_t st) {
  CPR_LDS_GUARD((k_mdp_pe_resident<PER, KEEP>), bytes);
  if (bytes > 64 * 1024) {
    const hipError_t e = hipFuncSetAttribute(
        (const void*)k_mdp_pe_resident<PER, KEEP>, hipFuncAttributeMaxDynamicSharedMemorySize,
        (int)std::min<int64_t>(lds_dynamic_max((const void*)k_mdp_pe_resident<PER, KEEP>),
                               160 * 1024 - 2048));
    if (e != hipSuccess) return e;
  }
  hipLaunchKernelGGL((k_mdp_pe_resident<PER, KEEP>), dim3((unsigned)R.E), dim3(threads),
                     (size_t)bytes, st, M, R);
  return hipGetLastError();
}

hipError_t launch_mdp_pe_resident(const MdpDev& M, const MdpPeRun& R, hipStream_t st) {
  if (!mdp_pe_resident_fits(M.S) || R.E < 1) return hipErrorInvalidValue;
  const int64_t bytes = (int64_t)mdp_resident_lds(M.S);
  const int threads = (int)std::min<int64_t>(kMdpThreads, (M.S + 63) / 64 * 64);
  const int64_t per = (M.S + threads - 1) / threads;
  if (!R.reread && mdp_pe_resident_keeps(M.S, M.T)) {
    if (per <= 1) return launch_mdp_pe_resident_per<1, true>(M, R, threads, bytes, st);
    return launch_mdp_pe_resident_per<2, true>(M, R, threads, bytes, st);
  }
  if (per <= 1) return launch_mdp_pe_resident_per<1, false>(M, R, threads, bytes, st);
  if (per <= 2) return launch_mdp_pe_resident_per<2, false>(M, R, threads, bytes, st);
  if (per <= 4) return launch_mdp_pe_resident_per<4, false>(M, R, threads, bytes, st);
  if (per <= kMdpPer) return launch_mdp_pe_resident_per<kMdpPer, false>(M, R, threads, bytes, st);
  return hipErrorInvalidValue;
}

hipError_t launch_mdp_pe_sweep(const MdpDev& M, const MdpPeRun& R, int64_t k, hipStream_t st) {
  const int64_t chunks = ((int64_t)M.S + kMdpBlock - 1) / kMdpBlock;
  if (k < 1 || R.E < 1 || chunks * R.E > INT32_MAX) return hipErrorInvalidValue;
  hipLaunchKernelGGL(k_mdp_pe_sweep, dim3((unsigned)(chunks * R.E)), dim3(kMdpBlock), 0, st, M, R,
                     k, (int32_t)chunks);
  return hipGetLastError();
}

}  // namespace cpr
