// The dense layer of the neural-network policy kernels on the f32-input MFMA, shared by the
// rollout's forward (kernels_policy.hip) and the learner's forward with saved activations
// (kernels_ppo.hip). DESIGN.md §4.14.
#pragma once
#include <hip/hip_runtime.h>

#include "cpr_stream.h"
#include "policy_net.h"

#pragma clang fp contract(off)

namespace cpr {

using f32x4 = __attribute__((ext_vector_type(4))) float;

extern __shared__ __attribute__((aligned(16))) float pol_lds[];

// threads of a k_policy_forward workgroup: eight waves, two per SIMD, so that one wave's
// barrier and LDS waits overlap the other's MFMAs
constexpr int kPolThreads = 512;

// dst[r][c] = act(sum_k src[r][k] W[c][k] + b[c]) for the workgroup's kPolRows rows.
// src / dst are LDS tiles (src zero-filled up to the next multiple of 4 columns); W is staged
// through `ws` in chunks of kPolNT output units x kPolKT inputs, zero beyond n_out / n_in.
// Wave w owns the 16 output units n0 + 16 (w & 3) .. of a chunk for the 32 rows of half
// w >> 2: two 16x16 accumulators. Operand lane maps of the 16x16x4 f32 MFMA: A[lane & 15][k = lane >> 4],
// B[k = lane >> 4][lane & 15]; C/D column = lane & 15, row = 4 (lane >> 4) + register.
__device__ inline void pol_layer(const float* src, int sstride, const PolLayer& Ly, float* ws,
                                 float* dst, int dstride, bool relu) {
  constexpr int kStage = kPolNT * kPolKT / kPolThreads;  // weights a thread stages per chunk
  const int tid = (int)threadIdx.x, lane = tid & 63, wave = (tid >> 6) & 3, half = tid >> 8;
  const int K = Ly.n_in, N = Ly.n_out;
  const int Kp = (K + 3) & ~3;
  const int r16 = lane & 15, q = lane >> 4;
  const int kch = (Kp + kPolKT - 1) / kPolKT;
  const int total = ((N + kPolNT - 1) / kPolNT) * kch;
  // chunk c = (n-chunk c / kch, k-chunk c % kch); its weights travel global -> registers ->
  // LDS, and the loads of chunk c + 1 are in flight while chunk c is multiplied
  float stage[kStage];
  auto fetch = [&](int c) {
    const int n0 = (c / kch) * kPolNT, k0 = (c % kch) * kPolKT;
#pragma unroll
    for (int i = 0; i < kStage; ++i) {
      const int idx = tid + i * kPolThreads;
      const int o = n0 + idx / kPolKT, k = k0 + idx % kPolKT;
      stage[i] = (o < N && k < K) ? Ly.W[(int64_t)o * K + k] : 0.f;
    }
  };
  fetch(0);
  f32x4 acc[2];
  for (int c = 0; c < total; ++c) {
    const int n0 = (c / kch) * kPolNT, k0 = (c % kch) * kPolKT;
    __syncthreads();  // the previous chunk is consumed; src is complete
#pragma unroll
    for (int i = 0; i < kStage; ++i) {
      const int idx = tid + i * kPolThreads;
      ws[(idx / kPolKT) * kPolWsStride + idx % kPolKT] = stage[i];
    }
    __syncthreads();
    if (c + 1 < total) fetch(c + 1);
    const bool active = n0 + wave * 16 < N;  // wave-uniform
    if (k0 == 0) {
#pragma unroll
      for (int rb = 0; rb < 2; ++rb) acc[rb] = f32x4{0.f, 0.f, 0.f, 0.f};
    }
    if (active) {
      const float* wrow = ws + (wave * 16 + r16) * kPolWsStride + q;
      const float* arow = src + (half * 32 + r16) * sstride + k0 + q;
      if (Kp - k0 >= kPolKT) {
#pragma unroll
        for (int kk = 0; kk < kPolKT; kk += 4) {
          const float b = wrow[kk];
#pragma unroll
          for (int rb = 0; rb < 2; ++rb)
            acc[rb] = __builtin_amdgcn_mfma_f32_16x16x4f32(arow[rb * 16 * sstride + kk], b,
                                                           acc[rb], 0, 0, 0);
        }
      } else {
        for (int kk = 0; kk < Kp - k0; kk += 4) {
          const float b = wrow[kk];
#pragma unroll
          for (int rb = 0; rb < 2; ++rb)
            acc[rb] = __builtin_amdgcn_mfma_f32_16x16x4f32(arow[rb * 16 * sstride + kk], b,
                                                           acc[rb], 0, 0, 0);
        }
      }
    }
    const int col = n0 + wave * 16 + r16;
    if (k0 + kPolKT >= Kp && active && col < N) {  // the n-chunk's last k-chunk
      const float bias = Ly.b[col];
#pragma unroll
      for (int rb = 0; rb < 2; ++rb)
#pragma unroll
        for (int g = 0; g < 4; ++g) {
          float v = acc[rb][g] + bias;
          if (relu) v = v < 0.f ? 0.f : v;
          dst[(half * 32 + rb * 16 + q * 4 + g) * dstride + col] = v;
        }
    }
  }
  __syncthreads();
}

// The forward's epilogue for one row, shared by k_policy_forward and the one-kernel FC16
// rollout (k_fc16_rollout_net): from the row's f32 logits `l` the action (the lowest index of
// the maximum, or the keyed sample at the draw key() returns) and its log-probability in f64.
// key() -> Stream and step index of the row's draw; called only when sampling.
struct PolChoice {
  int32_t action;
  double logp;
};

template <class Key>
__device__ inline PolChoice pol_choose(const float* l, int na, bool deterministic, Key key) {
  float mf = l[0];
  int am = 0;
  for (int i = 1; i < na; ++i)
    if (l[i] > mf) {  // the lowest index of the maximum
      mf = l[i];
      am = i;
    }
  const double m = (double)mf;
  double S = 0.0;
  for (int i = 0; i < na; ++i) S += exp((double)l[i] - m);
  int a = am;
  if (!deterministic) {
    // u of the keyed block (episode, step index, TAG_POLICY): the smallest a with
    // u S < sum_{i <= a} e_i, the last action if rounding leaves none
    uint32_t si = 0u;
    const Stream st = key(&si);
    const Words4 w = st.block(si, TAG_POLICY);
    const double uS = u53(w.w0, w.w1) * S;
    double c = 0.0;
    a = na - 1;
    for (int i = 0; i < na; ++i) {
      c += exp((double)l[i] - m);
      if (uS < c) {
        a = i;
        break;
      }
    }
  }
  return PolChoice{a, ((double)l[a] - m) - log(S)};
}

}  // namespace cpr
