// gfx950 kernels of the learner (ppo.h, DESIGN.md §4.14 "Learner"):
//   k_gae           generalised advantage estimation, one thread per lane
//   k_adv_part      partial sums of the minibatch's advantages (f64, fixed order)
//   k_adv_norm      the minibatch's advantages, gathered and normalised
//   k_ppo_forward   k_policy_forward's MLP over gathered rows with every hidden activation
//                   saved to HBM, then the PPO loss and its derivative per row in f64
//   k_ppo_stats     the minibatch's statistics from the workgroups' partials
//   k_ppo_dw        dW = dY^T X and db = sum dY of one layer, per row block, on the MFMA
//   k_ppo_dx        dX = (X > 0) dY W of one layer on the MFMA
//   k_ppo_reduce, k_ppo_reduce_bias  the row blocks' partials summed in block order
//   k_grad_sq       partial sums of squares of the gradient (f64, fixed order)
//   k_grad_norm     the gradient's global L2 norm from them
//   k_adam          the norm clip and Adam, elementwise f32
// No floating-point atomics anywhere: every sum has one order, so a call repeats bit for bit.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "kernels.h"
#include "policy_layer.h"
#include "policy_net.h"
#include "ppo.h"

#pragma clang fp contract(off)

namespace cpr {

__global__ __launch_bounds__(kBlock) void k_gae(int64_t n_steps, int64_t n, const double* reward,
                                                const uint8_t* done, const double* value,
                                                double gamma, double lam, double* adv,
                                                double* ret) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const double gl = gamma * lam;
  double last = 0.0;
  double v1 = value[n_steps * n + i];
  for (int64_t t = n_steps - 1; t >= 0; --t) {
    const int64_t c = t * n + i;
    const double nnt = 1.0 - (done[c] ? 1.0 : 0.0);
    const double v0 = value[c];
    const double delta = (reward[c] + (gamma * v1) * nnt) - v0;
    last = delta + (gl * nnt) * last;
    adv[c] = last;
    ret[c] = last + v0;
    v1 = v0;
  }
}

// sum of v over the workgroup: a binary tree over the threads' values, the same for every run
__device__ inline double red_sum(double v, double* red) {
  const int tid = (int)threadIdx.x;
  __syncthreads();  // red's previous readers
  red[tid] = v;
  __syncthreads();
  for (int o = kPpoRedThreads / 2; o > 0; o >>= 1) {
    if (tid < o) red[tid] = red[tid] + red[tid + o];
    __syncthreads();
  }
  return red[0];
}

// a row index of the flat buffers; anything outside [0, N) reads row 0 instead of memory
// that is not the caller's
__device__ inline int64_t ppo_row(const int32_t* idx, int64_t i, int64_t N) {
  const int64_t g = idx[i];
  return (uint64_t)g < (uint64_t)N ? g : 0;
}

// The f64 reductions over many elements (a minibatch's advantages, the gradient) run in two
// stages with one order: workgroup g sums elements [g, g + 1) * chunk, thread-strided and then by
// the tree, into partial[g]; the partials are added in workgroup order.
__device__ inline double red_partials(const double* partial, int blocks) {
  double s = 0.0;
  for (int g = 0; g < blocks; ++g) s += partial[g];
  return s;
}

// pass 0: partial sums of the gathered advantages; pass 1: of their squared distances from the
// mean of pass 0's partials
__global__ __launch_bounds__(kPpoRedThreads) void k_adv_part(const double* adv, const int32_t* idx,
                                                             int64_t B, int64_t N, int64_t chunk,
                                                             int pass, const double* psum,
                                                             double* pout) {
  __shared__ double red[kPpoRedThreads];
  const int64_t beg = (int64_t)blockIdx.x * chunk, end = beg + chunk < B ? beg + chunk : B;
  const double mean = pass ? red_partials(psum, (int)gridDim.x) / (double)B : 0.0;
  double s = 0.0;
  for (int64_t i = beg + threadIdx.x; i < end; i += kPpoRedThreads) {
    const double d = adv[ppo_row(idx, i, N)] - mean;
    s += pass ? d * d : d;
  }
  s = red_sum(s, red);
  if (threadIdx.x == 0) pout[blockIdx.x] = s;
}

__global__ __launch_bounds__(kPpoRedThreads) void k_adv_norm(const double* adv, const int32_t* idx,
                                                             int64_t B, int64_t N, int normalize,
                                                             const double* psum, const double* psq,
                                                             int blocks, double* out) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= B) return;
  const double a = adv[ppo_row(idx, i, N)];
  if (!normalize) {
    out[i] = a;
    return;
  }
  const double mean = red_partials(psum, blocks) / (double)B;
  const double sd = sqrt(red_partials(psq, blocks) / (double)(B - 1));
  out[i] = (a - mean) / (sd + 1e-8);
}

__global__ __launch_bounds__(kPolThreads) void k_ppo_forward(PolNet N, PpoFwd F, int32_t hstride) {
  float* xin = pol_lds;
  float* ws = xin + kPolRows * kPolInStride;
  float* lg = ws + kPolNT * kPolWsStride;
  float* val = lg + kPolRows * kPolLogitStride;
  float* h0 = val + kPolRows;
  float* h1 = h0 + kPolRows * hstride;  // used from depth 2 on (policy_lds_bytes)
  const int tid = (int)threadIdx.x;
  const int64_t r0 = (int64_t)blockIdx.x * kPolRows;
  const int n_in = N.obs_len + N.n_extra;
  // the input tile as in k_policy_forward, of the gathered rows; kept for the first layer's dW
  for (int idx = tid; idx < kPolRows * kPolInStride; idx += kPolThreads) {
    const int r = idx / kPolInStride, c = idx - r * kPolInStride;
    const int64_t row = r0 + r;
    float v = 0.f;
    if (row < F.B) {
      const int64_t g = ppo_row(F.idx, row, F.N);
      if (c < N.obs_len)
        v = (float)F.obs[g * N.obs_len + c];
      else if (c < n_in)
        v = (F.alpha && c - N.obs_len == F.alpha_col) ? (float)F.alpha[g] : N.extra[c - N.obs_len];
      F.xin[row * kPolInStride + c] = v;
    }
    xin[idx] = v;
  }
  for (int trunk = 0; trunk < 2; ++trunk) {
    const PolLayer* Ls = trunk == 0 ? N.pi : N.vf;
    const int width = trunk == 0 ? N.width_pi : N.width_vf;
    const float* src = xin;
    int sstride = kPolInStride;
    for (int l = 0; l < N.depth; ++l) {
      float* dst = (l & 1) ? h1 : h0;
      pol_layer(src, sstride, Ls[l], ws, dst, hstride, true);
      // the tile is complete (pol_layer ends on a barrier); its next writer is layer l + 2,
      // a whole pol_layer and its barriers away
      float* save = F.act[trunk][l];
      for (int idx = tid; idx < kPolRows * width; idx += kPolThreads) {
        const int r = idx / width, c = idx - r * width;
        if (r0 + r < F.B) save[(r0 + r) * width + c] = dst[r * hstride + c];
      }
      src = dst;
      sstride = hstride;
    }
    if (trunk == 0)
      pol_layer(src, sstride, Ls[N.depth], ws, lg, kPolLogitStride, false);
    else
      pol_layer(src, sstride, Ls[N.depth], ws, val, 1, false);
  }
  // the loss and its derivative, one thread per row; the weight chunk's space now holds the
  // rows' statistics (pol_layer's last barrier is behind every reader of ws)
  double* rs = (double*)ws;  // [kPpoRowStats][kPolRows]
  const int64_t row = r0 + tid;
  if (tid < kPolRows) {
    double st[kPpoRowStats] = {0.0, 0.0, 0.0, 0.0, 0.0};
    if (row < F.B) {
      const int64_t g = ppo_row(F.idx, row, F.N);
      const float* l = lg + tid * kPolLogitStride;
      const int na = N.n_actions;
      int a = F.action[g];
      a = a < 0 ? 0 : (a >= na ? na - 1 : a);
      float mf = l[0];
      for (int i = 1; i < na; ++i)
        if (l[i] > mf) mf = l[i];
      const double m = (double)mf;
      double S = 0.0;
      for (int i = 0; i < na; ++i) S += exp((double)l[i] - m);
      const double logS = log(S);
      const double logp = ((double)l[a] - m) - logS;
      const double lr = logp - F.old_logp[g];
      const double rho = exp(lr);
      const double A = F.advn[row];
      const double lo = 1.0 - F.clip, hi = 1.0 + F.clip;
      const double rc = rho < lo ? lo : (rho > hi ? hi : rho);
      const double s1 = A * rho, s2 = A * rc;
      const bool clipped = (A > 0.0 && rho > hi) || (A < 0.0 && rho < lo);
      const double g_logp = clipped ? 0.0 : -s1;
      double H = 0.0;
      for (int i = 0; i < na; ++i) {
        const double lpi = ((double)l[i] - m) - logS;
        H -= exp(lpi) * lpi;
      }
      const double invB = 1.0 / (double)F.B;
      for (int i = 0; i < na; ++i) {
        const double lpi = ((double)l[i] - m) - logS;
        const double p = exp(lpi);
        const double d = g_logp * ((i == a ? 1.0 : 0.0) - p) + F.ent_coef * (p * (lpi + H));
        F.dlogits[row * na + i] = (float)(d * invB);
      }
      const double v = (double)val[tid], R = F.ret[g];
      F.dvalue[row] = (float)(((2.0 * F.vf_coef) * (v - R)) * invB);
      st[kPpoPolicyLoss] = -(s1 < s2 ? s1 : s2);
      st[kPpoValueLoss] = (R - v) * (R - v);
      st[kPpoEntropyLoss] = -H;
      st[kPpoApproxKl] = (rho - 1.0) - lr;
      st[kPpoClipFraction] = fabs(rho - 1.0) > F.clip ? 1.0 : 0.0;
    }
    for (int k = 0; k < kPpoRowStats; ++k) rs[k * kPolRows + tid] = st[k];
  }
  __syncthreads();
  if (tid < kPpoRowStats) {
    double s = 0.0;
    for (int r = 0; r < kPolRows; ++r) s += rs[tid * kPolRows + r];
    F.partial[(int64_t)blockIdx.x * kPpoRowStats + tid] = s;
  }
}

__global__ __launch_bounds__(64) void k_ppo_stats(const double* partial, int64_t blocks, int64_t B,
                                                  double ent_coef, double vf_coef, double* stats,
                                                  double* acc) {
  __shared__ double mean[kPpoRowStats];
  const int tid = (int)threadIdx.x;
  if (tid < kPpoRowStats) {
    double s = 0.0;
    for (int64_t b = 0; b < blocks; ++b) s += partial[b * kPpoRowStats + tid];
    mean[tid] = s / (double)B;
  }
  __syncthreads();
  if (tid < kPpoRowStats) {
    stats[tid] = mean[tid];
    if (acc) acc[tid] += mean[tid];
  } else if (tid == kPpoLoss) {
    const double loss = (mean[kPpoPolicyLoss] + ent_coef * mean[kPpoEntropyLoss]) +
                        vf_coef * mean[kPpoValueLoss];
    stats[kPpoLoss] = loss;
    if (acc) acc[kPpoLoss] += loss;
  }
}

// Operand lane maps of the 16x16x4 f32 MFMA as in pol_layer: A[lane & 15][k = lane >> 4],
// B[k = lane >> 4][lane & 15]; C/D column = lane & 15, row = 4 (lane >> 4) + register.
constexpr int kBwdThreads = 256;  // four waves
constexpr int kBwdTile = 64;      // output tile edge of k_ppo_dw and k_ppo_dx
constexpr int kBwdChunk = 32;     // reduction extent staged per pass
// floats per LDS row whose 64 columns an operand read walks along lane & 15 while lane >> 4
// walks rows: 80 = 16 mod 64, so the four rows of a read fall on the four bank quarters
constexpr int kBwdColStride = kBwdTile + 16;
// floats per LDS row whose rows a read walks along lane & 15 and columns along lane >> 4:
// 36 r + q covers the 64 banks once (pol_layer's width + 4 rule)
constexpr int kBwdRowStride = kBwdChunk + 4;

// dW[o][k] = sum_r dY[r][o] X[r][k]: the MFMA's A is dY^T (o along lane & 15, r along k), its
// B is X (r along k, k along lane & 15). A workgroup owns a 64 x 64 tile of dW for one row
// block; wave w the 16 output units o0 + 16 w .. and all 64 inputs (four accumulators). The
// tile at k0 = 0 also sums its dY columns into db, rows in order, in f64 (bpart).
__global__ __launch_bounds__(kBwdThreads) void k_ppo_dw(PpoBwd P) {
  __shared__ float ys[kBwdChunk * kBwdColStride];
  __shared__ float xs[kBwdChunk * kBwdColStride];
  const PpoBwdJob& J = P.j[blockIdx.z];
  const int kt_n = (J.n_in + kBwdTile - 1) / kBwdTile;
  const int ot_n = (J.n_out + kBwdTile - 1) / kBwdTile;
  if ((int)blockIdx.y >= kt_n * ot_n) return;  // the narrower trunk has fewer tiles
  const int o0 = ((int)blockIdx.y / kt_n) * kBwdTile, k0 = ((int)blockIdx.y % kt_n) * kBwdTile;
  const int tid = (int)threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int r16 = lane & 15, q = lane >> 4;
  const int64_t rbeg = (int64_t)blockIdx.x * P.rows_per_block;
  const int64_t rend = std::min<int64_t>(P.B, rbeg + P.rows_per_block);
  f32x4 acc[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) acc[j] = f32x4{0.f, 0.f, 0.f, 0.f};
  double bsum = 0.0;  // db sums signed terms that cancel: f64, rounded once per row block
  for (int64_t r0 = rbeg; r0 < rend; r0 += kBwdChunk) {
    __syncthreads();  // the previous chunk is consumed
    for (int i = tid; i < kBwdChunk * kBwdTile; i += kBwdThreads) {
      const int r = i / kBwdTile, c = i % kBwdTile;
      const int64_t row = r0 + r;
      const bool in = row < rend;
      ys[r * kBwdColStride + c] = (in && o0 + c < J.n_out) ? J.dY[row * J.ldy + o0 + c] : 0.f;
      xs[r * kBwdColStride + c] = (in && k0 + c < J.n_in) ? J.X[row * J.ldx + k0 + c] : 0.f;
    }
    __syncthreads();
    if (k0 == 0 && tid < kBwdTile)
      for (int r = 0; r < kBwdChunk; ++r) bsum += (double)ys[r * kBwdColStride + tid];
#pragma unroll
    for (int rr = 0; rr < kBwdChunk; rr += 4) {
      const float a = ys[(rr + q) * kBwdColStride + wave * 16 + r16];
#pragma unroll
      for (int j = 0; j < 4; ++j)
        acc[j] = __builtin_amdgcn_mfma_f32_16x16x4f32(a, xs[(rr + q) * kBwdColStride + j * 16 + r16],
                                                      acc[j], 0, 0, 0);
    }
  }
  float* part = P.part + (int64_t)blockIdx.x * P.pstride;
#pragma unroll
  for (int j = 0; j < 4; ++j)
#pragma unroll
    for (int g = 0; g < 4; ++g) {
      const int o = o0 + wave * 16 + q * 4 + g, k = k0 + j * 16 + r16;
      if (o < J.n_out && k < J.n_in) part[J.off_w + (int64_t)o * J.n_in + k] = acc[j][g];
    }
  if (k0 == 0 && tid < kBwdTile && o0 + tid < J.n_out)
    P.bpart[(int64_t)blockIdx.x * P.bstride + J.off_bc + o0 + tid] = bsum;
}

// dX[r][k] = (X[r][k] > 0) sum_o dY[r][o] W[o][k]: A is dY (rows along lane & 15, o along k),
// B is W (o along k, k along lane & 15). A workgroup owns 64 rows x 64 inputs; wave w the 16
// rows r0 + 16 w .. Rows beyond B are zero in the tile and never stored.
__global__ __launch_bounds__(kBwdThreads) void k_ppo_dx(PpoBwd P) {
  __shared__ float ys[kBwdTile * kBwdRowStride];
  __shared__ float wt[kBwdChunk * kBwdColStride];
  const PpoBwdJob& J = P.j[blockIdx.z];
  const int k0 = (int)blockIdx.y * kBwdTile;
  if (J.dX == nullptr || k0 >= J.n_in) return;
  const int tid = (int)threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int r16 = lane & 15, q = lane >> 4;
  const int64_t r0 = (int64_t)blockIdx.x * kBwdTile;
  f32x4 acc[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) acc[j] = f32x4{0.f, 0.f, 0.f, 0.f};
  for (int o0 = 0; o0 < J.n_out; o0 += kBwdChunk) {
    __syncthreads();
    for (int i = tid; i < kBwdTile * kBwdChunk; i += kBwdThreads) {
      const int r = i / kBwdChunk, c = i % kBwdChunk;
      const int64_t row = r0 + r;
      ys[r * kBwdRowStride + c] =
          (row < P.B && o0 + c < J.n_out) ? J.dY[row * J.ldy + o0 + c] : 0.f;
    }
    for (int i = tid; i < kBwdChunk * kBwdTile; i += kBwdThreads) {
      const int o = i / kBwdTile, c = i % kBwdTile;
      wt[o * kBwdColStride + c] = (o0 + o < J.n_out && k0 + c < J.n_in)
                                      ? J.W[(int64_t)(o0 + o) * J.n_in + k0 + c]
                                      : 0.f;
    }
    __syncthreads();
    const int od = std::min(kBwdChunk, (J.n_out - o0 + 3) & ~3);  // heads narrower than a chunk
    for (int oo = 0; oo < od; oo += 4) {
      const float a = ys[(wave * 16 + r16) * kBwdRowStride + oo + q];
#pragma unroll
      for (int j = 0; j < 4; ++j)
        acc[j] = __builtin_amdgcn_mfma_f32_16x16x4f32(a, wt[(oo + q) * kBwdColStride + j * 16 + r16],
                                                      acc[j], 0, 0, 0);
    }
  }
#pragma unroll
  for (int j = 0; j < 4; ++j)
#pragma unroll
    for (int g = 0; g < 4; ++g) {
      const int64_t row = r0 + wave * 16 + q * 4 + g;
      const int k = k0 + j * 16 + r16;
      if (row < P.B && k < J.n_in)
        J.dX[row * J.n_in + k] = J.X[row * J.ldx + k] > 0.f ? acc[j][g] : 0.f;
    }
}

__global__ __launch_bounds__(kBlock) void k_ppo_reduce(const float* part, int64_t pstride,
                                                       int32_t blocks, int64_t n, float* grad) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  double s = (double)part[i];
  for (int32_t b = 1; b < blocks; ++b) s += (double)part[(int64_t)b * pstride + i];
  grad[i] = (float)s;
}

__global__ __launch_bounds__(kBlock) void k_ppo_reduce_bias(const double* bpart, int64_t bstride,
                                                            int32_t blocks, PpoBiasMap M,
                                                            float* grad) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= M.start[M.arrays]) return;
  int k = 0;
  while (k + 1 < M.arrays && i >= M.start[k + 1]) ++k;
  double s = bpart[i];
  for (int32_t b = 1; b < blocks; ++b) s += bpart[(int64_t)b * bstride + i];
  grad[M.off[k] + (i - M.start[k])] = (float)s;
}

__global__ __launch_bounds__(kPpoRedThreads) void k_grad_sq(const float* grad, int64_t n,
                                                            int64_t chunk, double* pout) {
  __shared__ double red[kPpoRedThreads];
  const int64_t beg = (int64_t)blockIdx.x * chunk, end = beg + chunk < n ? beg + chunk : n;
  double s = 0.0;
  for (int64_t i = beg + threadIdx.x; i < end; i += kPpoRedThreads) {
    const double g = (double)grad[i];
    s += g * g;
  }
  s = red_sum(s, red);
  if (threadIdx.x == 0) pout[blockIdx.x] = s;
}

__global__ void k_grad_norm(const double* partial, int blocks, double* stats, double* acc) {
  const double norm = sqrt(red_partials(partial, blocks));
  stats[kPpoGradNorm] = norm;
  if (acc) acc[kPpoGradNorm] += norm;
}

__global__ __launch_bounds__(kBlock) void k_adam(PpoAdam A) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= A.n) return;
  float coef = A.max_norm / ((float)A.stats[kPpoGradNorm] + 1e-6f);
  coef = coef > 1.f ? 1.f : coef;
  const float g = A.g[i] * coef;
  const float m = A.b1 * A.m[i] + A.omb1 * g;
  const float v = A.b2 * A.v[i] + (A.omb2 * g) * g;
  A.m[i] = m;
  A.v[i] = v;
  const float denom = sqrtf(v) / A.bc2_sqrt + A.eps;
  A.p[i] = A.p[i] - (A.step * m) / denom;
}

// ---------------------------------------------------------------- launchers

static unsigned blocks_of(int64_t n, int per) { return (unsigned)((n + per - 1) / per); }

hipError_t launch_gae(int64_t n_steps, int64_t n, const double* reward, const uint8_t* done,
                      const double* value, double gamma, double lam, double* adv, double* ret,
                      hipStream_t st) {
  hipLaunchKernelGGL(k_gae, dim3(blocks_of(n, kBlock)), dim3(kBlock), 0, st, n_steps, n, reward,
                     done, value, gamma, lam, adv, ret);
  return hipGetLastError();
}

// workgroups of a two-stage reduction over n elements and the elements of each
static int red_blocks(int64_t n, int64_t* chunk) {
  const int64_t blocks = std::min<int64_t>(kPpoRedBlocks, (n + 4095) / 4096);
  *chunk = (n + blocks - 1) / blocks;
  return (int)((n + *chunk - 1) / *chunk);
}

hipError_t launch_adv_norm(const double* adv, const int32_t* idx, int64_t B, int64_t N,
                           int normalize, double* red, double* out, hipStream_t st) {
  const int norm = normalize && B > 1;
  int64_t chunk = 0;
  const int blocks = red_blocks(B, &chunk);
  double* psum = red;
  double* psq = red + kPpoRedBlocks;
  if (norm)
    for (int pass = 0; pass < 2; ++pass)
      hipLaunchKernelGGL(k_adv_part, dim3((unsigned)blocks), dim3(kPpoRedThreads), 0, st, adv, idx,
                         B, N, chunk, pass, psum, pass ? psq : psum);
  hipLaunchKernelGGL(k_adv_norm, dim3(blocks_of(B, kPpoRedThreads)), dim3(kPpoRedThreads), 0, st,
                     adv, idx, B, N, norm, psum, psq, blocks, out);
  return hipGetLastError();
}

int64_t ppo_lds_limit() {
  return std::min<int64_t>(lds_dynamic_max((const void*)k_ppo_forward), 160 * 1024 - 2048);
}

hipError_t launch_ppo_forward(const PolNet& N, const PpoFwd& F, hipStream_t st) {
  if (F.B <= 0) return hipSuccess;
  const int64_t bytes = ppo_lds_bytes(N.depth, N.width_pi, N.width_vf);
  if (bytes > ppo_lds_limit()) return hipErrorInvalidValue;
  CPR_LDS_GUARD(k_ppo_forward, bytes);
  if (bytes > 64 * 1024) {
    const hipError_t e = hipFuncSetAttribute((const void*)k_ppo_forward,
                                             hipFuncAttributeMaxDynamicSharedMemorySize,
                                             (int)ppo_lds_limit());
    if (e != hipSuccess) return e;
  }
  const int32_t w = N.width_pi > N.width_vf ? N.width_pi : N.width_vf;
  hipLaunchKernelGGL(k_ppo_forward, dim3(blocks_of(F.B, kPolRows)), dim3(kPolThreads),
                     (size_t)bytes, st, N, F, (int32_t)policy_act_stride(w));
  return hipGetLastError();
}

hipError_t launch_ppo_stats(const double* partial, int64_t blocks, int64_t B, double ent_coef,
                            double vf_coef, double* stats, double* acc, hipStream_t st) {
  hipLaunchKernelGGL(k_ppo_stats, dim3(1), dim3(64), 0, st, partial, blocks, B, ent_coef, vf_coef,
                     stats, acc);
  return hipGetLastError();
}

hipError_t launch_ppo_dw(const PpoBwd& P, hipStream_t st) {
  int tiles = 0;
  for (const PpoBwdJob& J : P.j)
    tiles = std::max(tiles, ((J.n_in + kBwdTile - 1) / kBwdTile) * ((J.n_out + kBwdTile - 1) / kBwdTile));
  const unsigned rb = blocks_of(P.B, P.rows_per_block);
  hipLaunchKernelGGL(k_ppo_dw, dim3(rb, (unsigned)tiles, 2), dim3(kBwdThreads), 0, st, P);
  return hipGetLastError();
}

hipError_t launch_ppo_dx(const PpoBwd& P, hipStream_t st) {
  int kt = 0;
  for (const PpoBwdJob& J : P.j)
    if (J.dX) kt = std::max(kt, (J.n_in + kBwdTile - 1) / kBwdTile);
  if (kt == 0) return hipSuccess;
  hipLaunchKernelGGL(k_ppo_dx, dim3(blocks_of(P.B, kBwdTile), (unsigned)kt, 2), dim3(kBwdThreads),
                     0, st, P);
  return hipGetLastError();
}

hipError_t launch_ppo_reduce(const float* part, int64_t pstride, int32_t blocks, int64_t n,
                             float* grad, hipStream_t st) {
  hipLaunchKernelGGL(k_ppo_reduce, dim3(blocks_of(n, kBlock)), dim3(kBlock), 0, st, part, pstride,
                     blocks, n, grad);
  return hipGetLastError();
}

hipError_t launch_ppo_reduce_bias(const double* bpart, int64_t bstride, int32_t blocks,
                                  const PpoBiasMap& M, float* grad, hipStream_t st) {
  hipLaunchKernelGGL(k_ppo_reduce_bias, dim3(blocks_of(M.start[M.arrays], kBlock)), dim3(kBlock),
                     0, st, bpart, bstride, blocks, M, grad);
  return hipGetLastError();
}

hipError_t launch_grad_norm(const float* grad, int64_t n, double* red, double* stats, double* acc,
                            hipStream_t st) {
  int64_t chunk = 0;
  const int blocks = red_blocks(n, &chunk);
  hipLaunchKernelGGL(k_grad_sq, dim3((unsigned)blocks), dim3(kPpoRedThreads), 0, st, grad, n, chunk,
                     red);
  hipLaunchKernelGGL(k_grad_norm, dim3(1), dim3(1), 0, st, (const double*)red, blocks, stats, acc);
  return hipGetLastError();
}

hipError_t launch_adam(const PpoAdam& A, hipStream_t st) {
  hipLaunchKernelGGL(k_adam, dim3(blocks_of(A.n, kBlock)), dim3(kBlock), 0, st, A);
  return hipGetLastError();
}

}  // namespace cpr
