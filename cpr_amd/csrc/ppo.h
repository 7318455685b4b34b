// Parameter structs and launchers of the learner's kernels (kernels_ppo.hip): generalised
// advantage estimation, the forward with saved activations and the PPO loss epilogue, the
// backward on the f32 MFMA, the global-norm clip and Adam. DESIGN.md §4.14 "Learner".
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include "policy_net.h"

namespace cpr {

// per-minibatch statistics on the device, f64: the first five are row means
enum {
  kPpoPolicyLoss = 0,
  kPpoValueLoss = 1,
  kPpoEntropyLoss = 2,
  kPpoApproxKl = 3,
  kPpoClipFraction = 4,
  kPpoLoss = 5,      // policy + ent_coef entropy + vf_coef value
  kPpoGradNorm = 6,  // global L2 norm of the gradient before the clip
  kPpoStats = 8
};
constexpr int kPpoRowStats = 5;      // statistics summed over rows (per-workgroup partials)
constexpr int kPpoMaxRowBlocks = 32; // row blocks of the weight gradient's partial sums
constexpr int kPpoRedThreads = 256;  // threads of a workgroup of the f64 reductions
constexpr int kPpoRedBlocks = 128;   // most workgroups (partials) of one f64 reduction

// SB3's RolloutBuffer.compute_returns_and_advantage over step-major [n_steps][n] buffers
// (value has n_steps + 1 rows). Per lane, t = n_steps - 1 .. 0, one rounding per operation:
//   nnt = 1 - done[t]
//   delta = (reward[t] + (gamma * value[t + 1]) * nnt) - value[t]
//   last = delta + ((gamma * lam) * nnt) * last
//   adv[t] = last, ret[t] = last + value[t]
hipError_t launch_gae(int64_t n_steps, int64_t n, const double* reward, const uint8_t* done,
                      const double* value, double gamma, double lam, double* adv, double* ret,
                      hipStream_t st);

// out[i] = adv[idx[i]], i < B; with normalize != 0 and B > 1, (a - mean) / (std + 1e-8) with the
// unbiased std: two passes in f64, each in one fixed order (per workgroup of up to
// ceil(B / 4096) <= kPpoRedBlocks a contiguous chunk, thread-strided sums and a binary tree;
// then the workgroups' partials in order). red: 2 kPpoRedBlocks doubles of scratch
hipError_t launch_adv_norm(const double* adv, const int32_t* idx, int64_t B, int64_t N,
                           int normalize, double* red, double* out, hipStream_t st);

// the forward over the minibatch's rows idx[0 .. B) of the flat rollout buffers, the saved
// activations and the loss epilogue
struct PpoFwd {
  const double* obs;       // [N][obs_len]
  const double* alpha;     // [N] lane alpha of each row; null: the constants
  int32_t alpha_col;
  const int32_t* action;   // [N]
  const double* old_logp;  // [N]
  const double* ret;       // [N]
  const double* advn;      // [B] minibatch order (launch_adv_norm)
  const int32_t* idx;      // [B] rows of the minibatch
  int64_t B, N;
  double clip, ent_coef, vf_coef;
  float* xin;                      // [B][kPolInStride] the f32 input rows
  float* act[2][kPolMaxDepth];     // [trunk][layer] [B][width] hidden activations
  float* dlogits;                  // [B][n_actions] dL/dlogits
  float* dvalue;                   // [B] dL/dvalue
  double* partial;                 // [workgroups][kPpoRowStats]
};
hipError_t launch_ppo_forward(const PolNet& N, const PpoFwd& F, hipStream_t st);
// stats[0 .. kPpoLoss] of the minibatch from the workgroups' partials (summed in workgroup
// order); acc (optional) += stats
hipError_t launch_ppo_stats(const double* partial, int64_t blocks, int64_t B, double ent_coef,
                            double vf_coef, double* stats, double* acc, hipStream_t st);

// one Linear layer's backward: Y = X W^T + b over the minibatch's rows
struct PpoBwdJob {
  const float* dY;  // [B][ldy] dL/dY (n_out columns used)
  const float* X;   // [B][ldx] the layer's input (n_in columns used)
  const float* W;   // [n_out][n_in]
  float* dX;        // [B][n_in] dL/dX masked by X > 0; null for the input layer
  int32_t ldy, ldx, n_out, n_in;
  int64_t off_w, off_b;  // where dW and db stand in the padded parameter layout (floats)
  int64_t off_bc;        // where db stands among the biases alone (bpart)
};
// the same layer of both trunks in one launch (blockIdx.z)
struct PpoBwd {
  PpoBwdJob j[2];
  int64_t B;
  int32_t rows_per_block;  // a multiple of 32; row block r covers rows [r, r + 1) * this
  float* part;             // [row blocks][pstride] partial dW of each row block
  int64_t pstride;
  double* bpart;           // [row blocks][bstride] partial db of each row block, f64
  int64_t bstride;
};
hipError_t launch_ppo_dw(const PpoBwd& P, hipStream_t st);
hipError_t launch_ppo_dx(const PpoBwd& P, hipStream_t st);
// grad[i] = sum over row blocks, in block order, of part[block][i] (f64, rounded once)
hipError_t launch_ppo_reduce(const float* part, int64_t pstride, int32_t blocks, int64_t n,
                             float* grad, hipStream_t st);
// the same for the biases, whose partials are f64 (a bias gradient is a plain sum of signed
// terms; an f32 partial per row block would cost it an ulp): bias array k holds the compact
// indices [start[k], start[k + 1]) and stands at grad + off[k]
struct PpoBiasMap {
  int32_t arrays;
  int64_t start[2 * (kPolMaxDepth + 1) + 1];
  int64_t off[2 * (kPolMaxDepth + 1)];
};
hipError_t launch_ppo_reduce_bias(const double* bpart, int64_t bstride, int32_t blocks,
                                  const PpoBiasMap& M, float* grad, hipStream_t st);
// stats[kPpoGradNorm] = sqrt(sum g^2) in f64, the same two-stage order; acc (optional) += it.
// red: kPpoRedBlocks doubles of scratch
hipError_t launch_grad_norm(const float* grad, int64_t n, double* red, double* stats, double* acc,
                            hipStream_t st);

// torch.nn.utils.clip_grad_norm_ and torch.optim.Adam on f32, elementwise:
//   g *= min(1, max_norm / (norm + 1e-6));  m = b1 m + (1 - b1) g;  v = b2 v + (1 - b2) g g
//   p -= (step m) / (sqrt(v) / bc2_sqrt + eps),  step = lr / (1 - b1^t), bc2_sqrt = sqrt(1 - b2^t)
struct PpoAdam {
  float* p;
  const float* g;
  float* m;
  float* v;
  int64_t n;
  const double* stats;  // the norm at stats[kPpoGradNorm]
  float max_norm, b1, omb1, b2, omb2, step, bc2_sqrt, eps;
};
hipError_t launch_adam(const PpoAdam& A, hipStream_t st);

// dynamic LDS of the training forward (k_ppo_forward): k_policy_forward's tiles; the loss
// epilogue's per-row statistics reuse the weight chunk's space
inline int64_t ppo_lds_bytes(int32_t depth, int32_t width_pi, int32_t width_vf) {
  return policy_lds_bytes(depth, width_pi, width_vf);
}
int64_t ppo_lds_limit();

}  // namespace cpr
