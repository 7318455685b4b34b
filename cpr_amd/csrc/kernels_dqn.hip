// gfx950 kernels of Q-learning (dqn.h, DESIGN.md §4.14 "Q-learning"):
//   k_dqn_act       k_policy_forward's pi trunk for a tile of lanes, then the epsilon-greedy
//                   action from the keyed stream; the f32 input row, the lane alpha and the
//                   action go straight into the replay slot of the step
//   k_dqn_store     the slot's next observation (f64 -> f32) after the masked reset
//   k_dqn_forward   the online network over gathered transitions with every hidden activation
//                   saved (k_ppo_forward's pi trunk), the target network on the next
//                   observations in the second trunk's place, then the TD target, the Huber
//                   loss and its derivative per row in f64
//   k_dqn_stats     a gradient step's statistics from the workgroups' partials
//   k_polyak        the target network's update
// The vf trunk is never evaluated. No floating-point atomics: every sum has one order.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "dqn.h"
#include "kernels.h"
#include "policy_layer.h"
#include "policy_net.h"
#include "summary.h"

#pragma clang fp contract(off)

namespace cpr {

// the LDS carve of k_policy_forward (policy_lds_bytes)
struct DqnTiles {
  float *xin, *ws, *lg, *h0, *h1;
};
__device__ inline DqnTiles dqn_tiles(int32_t hstride) {
  DqnTiles T;
  T.xin = pol_lds;
  T.ws = T.xin + kPolRows * kPolInStride;
  T.lg = T.ws + kPolNT * kPolWsStride;
  T.h0 = T.lg + kPolRows * kPolLogitStride + kPolRows;  // the value column stays unused
  T.h1 = T.h0 + kPolRows * hstride;  // used from depth 2 on
  return T;
}

__global__ __launch_bounds__(kPolThreads) void k_dqn_act(PolNet N, DqnAct A, int32_t hstride) {
  const DqnTiles T = dqn_tiles(hstride);
  const int tid = (int)threadIdx.x;
  const int64_t r0 = (int64_t)blockIdx.x * kPolRows;
  const int n_in = N.obs_len + N.n_extra;
  // the input tile as in k_policy_forward; its observation columns are the slot's obs row
  for (int idx = tid; idx < kPolRows * kPolInStride; idx += kPolThreads) {
    const int r = idx / kPolInStride, c = idx - r * kPolInStride;
    const int64_t row = r0 + r;
    float v = 0.f;
    if (row < A.n) {
      if (c < N.obs_len) {
        v = (float)A.obs[row * N.obs_len + c];
        A.slot.obs[row * N.obs_len + c] = v;
      } else if (c < n_in) {
        v = (A.lane_alpha && c - N.obs_len == A.alpha_col) ? (float)A.lane_alpha[row]
                                                           : N.extra[c - N.obs_len];
      }
    }
    T.xin[idx] = v;
  }
  const float* src = T.xin;
  int sstride = kPolInStride;
  for (int l = 0; l < N.depth; ++l) {
    float* dst = (l & 1) ? T.h1 : T.h0;
    pol_layer(src, sstride, N.pi[l], T.ws, dst, hstride, true);
    src = dst;
    sstride = hstride;
  }
  pol_layer(src, sstride, N.pi[N.depth], T.ws, T.lg, kPolLogitStride, false);
  const int64_t row = r0 + tid;
  if (tid >= kPolRows || row >= A.n) return;
  const float* l = T.lg + tid * kPolLogitStride;
  const int na = N.n_actions;
  float mf = l[0];
  int a = 0;
  for (int i = 1; i < na; ++i)
    if (l[i] > mf) {  // the lowest index of the maximum
      mf = l[i];
      a = i;
    }
  if (A.epsilon > 0.0) {
    const Words4 w = make_stream(A.seed, A.ep[row]).block((uint32_t)A.step[row], TAG_EXPLORE);
    if (u53(w.w0, w.w1) < A.epsilon) {
      const int r = (int)(u53(w.w2, w.w3) * (double)na);
      a = r < na - 1 ? r : na - 1;
    }
  }
  A.action[row] = a;
  A.slot.action[row] = a;
  A.slot.alpha[row] = A.lane_alpha ? A.lane_alpha[row] : A.cfg_alpha;
}

__global__ __launch_bounds__(kBlock) void k_dqn_store(const double* obs, int64_t cells,
                                                      float* next_obs) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < cells) next_obs[i] = (float)obs[i];
}

// a transition index; anything outside [0, N) reads row 0 instead of memory that is not the
// caller's
__device__ inline int64_t dqn_row(const int64_t* idx, int64_t i, int64_t N) {
  const int64_t g = idx[i];
  return (uint64_t)g < (uint64_t)N ? g : 0;
}

// N: the online network's pi trunk, and in the vf trunk's place the target network's pi trunk
__global__ __launch_bounds__(kPolThreads) void k_dqn_forward(PolNet N, DqnFwd F, int32_t hstride) {
  const DqnTiles T = dqn_tiles(hstride);
  const int tid = (int)threadIdx.x;
  const int64_t r0 = (int64_t)blockIdx.x * kPolRows;
  const int ol = N.obs_len, n_in = N.obs_len + N.n_extra, na = N.n_actions;
  const int width = N.width_pi;
  const int64_t row = r0 + tid;
  const bool owner = tid < kPolRows && row < F.B;
  const int64_t grow = owner ? dqn_row(F.idx, row, F.N) : 0;
  int a = 0;
  float qa = 0.f;
  // trunk 0: the online network on obs, activations saved; trunk 1: the target network on
  // next_obs, only the logits kept
  for (int trunk = 0; trunk < 2; ++trunk) {
    const PolLayer* Ls = trunk == 0 ? N.pi : N.vf;
    const float* o32 = trunk == 0 ? F.obs32 : F.next32;
    const double* o64 = trunk == 0 ? F.obs64 : F.next64;
    // (trunk 1: the tile's last readers, layer 0 of trunk 0, are behind pol_layer's barriers)
    for (int idx = tid; idx < kPolRows * kPolInStride; idx += kPolThreads) {
      const int r = idx / kPolInStride, c = idx - r * kPolInStride;
      const int64_t rw = r0 + r;
      float v = 0.f;
      if (rw < F.B) {
        const int64_t g = dqn_row(F.idx, rw, F.N);
        if (c < ol)
          v = o32 ? o32[g * ol + c] : (float)o64[g * ol + c];
        else if (c < n_in)
          v = (F.alpha && c - ol == F.alpha_col) ? (float)F.alpha[g] : N.extra[c - ol];
        if (trunk == 0) F.xin[rw * kPolInStride + c] = v;
      }
      T.xin[idx] = v;
    }
    const float* src = T.xin;
    int sstride = kPolInStride;
    for (int l = 0; l < N.depth; ++l) {
      float* dst = (l & 1) ? T.h1 : T.h0;
      pol_layer(src, sstride, Ls[l], T.ws, dst, hstride, true);
      if (trunk == 0) {
        // the tile is complete; its next writer is a whole pol_layer and its barriers away
        float* save = F.act[l];
        for (int idx = tid; idx < kPolRows * width; idx += kPolThreads) {
          const int r = idx / width, c = idx - r * width;
          if (r0 + r < F.B) save[(r0 + r) * width + c] = dst[r * hstride + c];
        }
      }
      src = dst;
      sstride = hstride;
    }
    pol_layer(src, sstride, Ls[N.depth], T.ws, T.lg, kPolLogitStride, false);
    if (trunk == 0 && owner) {
      // q_a stays in a register: the target's head overwrites the logits, after the barriers
      // of its hidden layers
      a = F.action[grow];
      a = a < 0 ? 0 : (a >= na ? na - 1 : a);
      qa = T.lg[tid * kPolLogitStride + a];
    }
  }
  // the TD target, the loss and its derivative, one thread per row; the weight chunk's space
  // holds the rows' statistics (pol_layer's last barrier is behind every reader of ws)
  double* rs = (double*)T.ws;  // [kDqnRowStats][kPolRows]
  if (tid < kPolRows) {
    double st[kDqnRowStats] = {0.0, 0.0, 0.0, 0.0};
    if (owner) {
      const float* l = T.lg + tid * kPolLogitStride;
      float qm = l[0];
      for (int i = 1; i < na; ++i)
        if (l[i] > qm) qm = l[i];
      const double nnt = 1.0 - (F.done[grow] ? 1.0 : 0.0);
      const double y = F.reward[grow] + (F.gamma * (double)qm) * nnt;
      const double d = (double)qa - y;
      const double ad = fabs(d);
      const double dc = d < -1.0 ? -1.0 : (d > 1.0 ? 1.0 : d);
      const float dq = (float)(dc / (double)F.B);
      for (int i = 0; i < na; ++i) F.dlogits[row * na + i] = i == a ? dq : 0.f;
      st[kDqnLoss] = ad < 1.0 ? 0.5 * (d * d) : ad - 0.5;
      st[kDqnAbsTd] = ad;
      st[kDqnQ] = (double)qa;
      st[kDqnTarget] = y;
    }
    for (int k = 0; k < kDqnRowStats; ++k) rs[k * kPolRows + tid] = st[k];
  }
  __syncthreads();
  if (tid < kDqnRowStats) {
    double s = 0.0;
    for (int r = 0; r < kPolRows; ++r) s += rs[tid * kPolRows + r];
    F.partial[(int64_t)blockIdx.x * kDqnRowStats + tid] = s;
  }
}

__global__ __launch_bounds__(64) void k_dqn_stats(const double* partial, int64_t blocks, int64_t B,
                                                  double* stats, double* acc) {
  const int tid = (int)threadIdx.x;
  if (tid >= kDqnRowStats) return;
  double s = 0.0;
  for (int64_t b = 0; b < blocks; ++b) s += partial[b * kDqnRowStats + tid];
  const double mean = s / (double)B;
  stats[tid] = mean;
  if (acc) acc[tid] += mean;
}

// four parameters per thread (the parameter buffers are multiples of four floats), then the rest
__global__ __launch_bounds__(kBlock) void k_polyak(float* t, const float* p, int64_t n, float omt,
                                                   float tf) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int64_t n4 = n / 4;
  if (i < n4) {
    const f32x4 pv = ((const f32x4*)p)[i];
    f32x4 tv = ((const f32x4*)t)[i];
#pragma unroll
    for (int k = 0; k < 4; ++k) tv[k] = omt == 0.f ? pv[k] : (tv[k] * omt) + (pv[k] * tf);
    ((f32x4*)t)[i] = tv;
  }
  const int64_t j = n4 * 4 + i;
  if (j < n) t[j] = omt == 0.f ? p[j] : (t[j] * omt) + (p[j] * tf);
}

// ---------------------------------------------------------------- launchers

static unsigned blocks_of(int64_t n, int per) { return (unsigned)((n + per - 1) / per); }

int64_t dqn_lds_limit() {
  const int64_t lim = std::min<int64_t>(lds_dynamic_max((const void*)k_dqn_act),
                                        lds_dynamic_max((const void*)k_dqn_forward));
  return std::min<int64_t>(lim, 160 * 1024 - 2048);
}

hipError_t launch_dqn_act(const PolNet& N, const DqnAct& A, hipStream_t st) {
  if (A.n <= 0) return hipSuccess;
  const int64_t bytes = policy_lds_bytes(N.depth, N.width_pi, N.width_vf);
  if (bytes > dqn_lds_limit()) return hipErrorInvalidValue;
  CPR_LDS_GUARD(k_dqn_act, bytes);
  if (bytes > 64 * 1024) {
    const hipError_t e = hipFuncSetAttribute(
        (const void*)k_dqn_act, hipFuncAttributeMaxDynamicSharedMemorySize, (int)dqn_lds_limit());
    if (e != hipSuccess) return e;
  }
  const int32_t w = N.width_pi > N.width_vf ? N.width_pi : N.width_vf;
  hipLaunchKernelGGL(k_dqn_act, dim3(blocks_of(A.n, kPolRows)), dim3(kPolThreads), (size_t)bytes,
                     st, N, A, (int32_t)policy_act_stride(w));
  return hipGetLastError();
}

hipError_t launch_dqn_store(const double* obs, int64_t cells, float* next_obs, hipStream_t st) {
  if (cells <= 0) return hipSuccess;
  hipLaunchKernelGGL(k_dqn_store, dim3(blocks_of(cells, kBlock)), dim3(kBlock), 0, st, obs, cells,
                     next_obs);
  return hipGetLastError();
}

hipError_t launch_dqn_forward(const PolNet& online, const PolNet& target, const DqnFwd& F,
                              hipStream_t st) {
  if (F.B <= 0) return hipSuccess;
  const int64_t bytes = policy_lds_bytes(online.depth, online.width_pi, online.width_vf);
  if (bytes > dqn_lds_limit()) return hipErrorInvalidValue;
  CPR_LDS_GUARD(k_dqn_forward, bytes);
  if (bytes > 64 * 1024) {
    const hipError_t e =
        hipFuncSetAttribute((const void*)k_dqn_forward,
                            hipFuncAttributeMaxDynamicSharedMemorySize, (int)dqn_lds_limit());
    if (e != hipSuccess) return e;
  }
  const int32_t w = online.width_pi > online.width_vf ? online.width_pi : online.width_vf;
  PolNet N = online;  // the target's pi trunk in the vf trunk's place
  for (int l = 0; l <= online.depth; ++l) N.vf[l] = target.pi[l];
  N.width_vf = online.width_pi;
  hipLaunchKernelGGL(k_dqn_forward, dim3(blocks_of(F.B, kPolRows)), dim3(kPolThreads),
                     (size_t)bytes, st, N, F, (int32_t)policy_act_stride(w));
  return hipGetLastError();
}

hipError_t launch_dqn_stats(const double* partial, int64_t blocks, int64_t B, double* stats,
                            double* acc, hipStream_t st) {
  hipLaunchKernelGGL(k_dqn_stats, dim3(1), dim3(64), 0, st, partial, blocks, B, stats, acc);
  return hipGetLastError();
}

hipError_t launch_polyak(float* t, const float* p, int64_t n, float omt, float tf, hipStream_t st) {
  if (n <= 0) return hipSuccess;
  hipLaunchKernelGGL(k_polyak, dim3(blocks_of(n / 4 + 3, kBlock)), dim3(kBlock), 0, st, t, p, n,
                     omt, tf);
  return hipGetLastError();
}

}  // namespace cpr
