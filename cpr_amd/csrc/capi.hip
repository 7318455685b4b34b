// libcpr_hip C ABI (include/cpr_hip.h): host side. Validation mirrors the reference's
// engine.ml:37-51 (Parameters.t) and network.ml:61-76 (selfish_mining) so invalid
// configurations fail with the same messages; all episode work runs on the device.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <memory>
#include <string>
#include <deque>
#include <vector>

#include "../../include/cpr_hip.h"
#include "dqn.h"
#include "eth_window.h"
#include "kernels.h"
#include "lane_env.h"
#include "mdp_vi.h"
#include "nak_hybrid.h"
#include "policy_net.h"
#include "ppo.h"

using namespace cpr;

#ifndef CPR_VERSION_STRING
#define CPR_VERSION_STRING "cpr-hip 0.1.0 (gfx950)"
#endif

static thread_local std::string g_err;

static int fail(int code, const std::string& msg) {
  g_err = msg;
  return code;
}

#define HIP_TRY(expr)                                                                    \
  do {                                                                                   \
    hipError_t e_ = (expr);                                                              \
    if (e_ != hipSuccess)                                                                \
      return fail(CPR_E_HIP, std::string(#expr " failed: ") + hipGetErrorString(e_));   \
  } while (0)

// device allocation owned by one object (freed on destruction, so every early return of
// an entry point releases its scratch buffers); not copyable
struct DevBuf {
  void* p = nullptr;
  size_t bytes = 0;
  DevBuf() = default;
  DevBuf(const DevBuf&) = delete;
  DevBuf& operator=(const DevBuf&) = delete;
  ~DevBuf() { release(); }
  hipError_t ensure(size_t n) {
    if (n <= bytes) return hipSuccess;
    if (p) (void)hipFree(p);
    p = nullptr;
    bytes = 0;
    hipError_t e = hipMalloc(&p, n);
    if (e == hipSuccess) bytes = n;
    return e;
  }
  void release() {
    if (p) (void)hipFree(p);
    p = nullptr;
    bytes = 0;
  }
};

struct cpr_ctx {
  int device;
  hipStream_t stream;
  int cus;
  // Nakamoto episodes flagged by the closed-form lane wait here for their exact re-run
  // (k_nak_exact_rerun), which runs at the next synchronization point, all of them in one
  // launch: rq = [kRerunQueue] int64 entries + a uint32 counter; one RerunLaunch per
  // episode-kernel launch since then
  DevBuf rq, rtab, rmem;
  // cpr_rerun_stats: per flush, HIP events around the re-run kernels and the count of
  // episodes the launches since the previous flush queued (copied to pinned host memory
  // before the counter is cleared; e2 follows that copy). Every flush folds the records
  // whose e2 has completed into rr_* and recycles them (drain_flush_recs), and waits for the
  // oldest when kFlushRecMax are outstanding, so a context that never asks for the stats
  // holds a bounded set of events and pinned words
  struct FlushRec {
    hipEvent_t e0 = nullptr, e1 = nullptr, e2 = nullptr;
    uint32_t* cnt = nullptr;  // pinned host word
  };
  std::deque<FlushRec> fl_pending;
  std::vector<FlushRec> fl_free;
  int64_t rr_episodes = 0, rr_flushes = 0;
  double rr_ms = 0.0;
  std::vector<RerunLaunch> rlaunch, rlaunch_up;
  // entries a launch may append (kRerunQueue; CPR_RERUN_QUEUE_CAP lowers it for tests);
  // an episode that finds the queue full waits in its launch's overflow flags: one byte
  // per episode of every launch since the last flush, carved from the chunks of `ovf` in
  // order (chunk ovf_chunk, ovf_used bytes taken). Chunks are never reallocated, so
  // filling one forces no flush until kOvfMaxChunks are in use (1 GiB of flags, ~200
  // launches of the bench's 5.2M episodes): a flush costs the latency of one exact episode
  // (~80 ms at the gym's 2016 steps), paid once per synchronization
  int64_t rq_cap = kRerunQueue;
  std::vector<std::unique_ptr<DevBuf>> ovf;
  size_t ovf_chunk = 0, ovf_used = 0;
  // per-lane scratch regions of fused-episode launches (event-engine rings and heaps, the
  // Nakamoto lane's spill / time log / tie-replay scratch), shared by every batch of the
  // context: launches on the context's stream run in order, so one grow-only pool serves an
  // alpha x gamma sweep of any number of batches
  DevBuf pool;
  // work-queue counter of the event-engine fused-episode launches (wave_sched.h
  // ev_next_episode), zeroed on the stream before each launch
  DevBuf wq;
  // the deferred-race kernels' eager second passes (kernels.hip launch_run_episodes) run on
  // `side`, behind their launch's main kernel, so that they overlap the next launch on
  // `stream`. Each reads one of two list buffers; list_ev[i] marks the end of the pass that
  // reads lists[i], and the next launch that writes lists[i] waits for it on `stream`.
  // side_join makes `stream` wait for every pass still pending (before a flush, a
  // synchronization, or any read of summaries and the re-run queue)
  hipStream_t side = nullptr;
  hipEvent_t main_ev = nullptr;
  DevBuf lists[2];
  hipEvent_t list_ev[2] = {nullptr, nullptr};
  bool list_pending[2] = {false, false};
  int list_i = 0;
  // cpr_run_episodes_async calls not launched yet: sweep points that share
  // seed, first episode, episode count and every parameter but alpha, to run in one lane of
  // k_run_episodes_fused. Launched by fuse_launch_pending, which every entry point calls first
  struct FuseMember {
    cpr_batch* b;
    cpr_summary* sum;
  };
  std::vector<FuseMember> fuse;
  int fuse_kind = 0;  // run_episodes_fusable of the members
  int64_t fuse_n = 0;
  uint64_t fuse_first = 0;
};

// the HIP events around a fused group's kernel, shared by its members (cpr_last_launch: the
// group's time divided by its size)
struct FuseTime {
  hipEvent_t ev0 = nullptr, ev1 = nullptr;
  int size = 1;
  ~FuseTime() {
    if (ev0) (void)hipEventDestroy(ev0);
    if (ev1) (void)hipEventDestroy(ev1);
  }
};

static hipError_t side_join(cpr_ctx* c) {
  for (int i = 0; i < 2; ++i)
    if (c->list_pending[i]) {
      const hipError_t e = hipStreamWaitEvent(c->stream, c->list_ev[i], 0);
      if (e != hipSuccess) return e;
      c->list_pending[i] = false;
    }
  return hipSuccess;
}

// the context's scratch pool with at least `bytes`
static hipError_t ctx_pool(cpr_ctx* c, size_t bytes, void** out) {
  hipError_t e = c->pool.ensure(bytes);
  *out = c->pool.p;
  return e;
}

// a zeroed work-queue counter for the next event-engine launch on the context's stream
// (launches on the stream run in order, so one counter serves them all)
static hipError_t ctx_next(cpr_ctx* c, unsigned long long** out) {
  hipError_t e = c->wq.ensure(8);
  if (e == hipSuccess) e = hipMemsetAsync(c->wq.p, 0, 8, c->stream);
  *out = (unsigned long long*)c->wq.p;
  return e;
}

static size_t align256(size_t x) { return (x + 255) & ~(size_t)255; }

struct cpr_batch {
  cpr_ctx* ctx;
  cpr_config cfg;
  NakParams P;
  eth::EthParams EP;     // CPR_PROTO_ETHEREUM
  bool is_eth = false;   // Ethereum lockstep lanes share bk_lmem / bk_slots
  bool nak_ev = false;   // Nakamoto on the event engine (nak_on_event_engine): Ethereum lanes
                         // in Nakamoto mode (EP)
  int64_t eth_bytes = 0;
  bk::BkParams BP;       // CPR_PROTO_BK
  DevBuf bk_lmem, bk_slots;  // lockstep lanes: n_lanes x bk_bytes, n_lanes slots
  int64_t bk_bytes = 0;
  ts::TsParams TP;       // CPR_PROTO_TAILSTORM (shares bk_lmem / bk_slots)
  fc16::Fc16Params FP;   // CPR_PROTO_FC16, CPR_PROTO_FC16_ENV
  bool is_fc16 = false;  // either of them: the fused-episode kernel k_fc16_episodes
  bool fc16_env = false; // CPR_PROTO_FC16_ENV: lockstep lanes over bk_slots (Fc16Slot)
  generic::GenericParams GP;  // CPR_PROTO_GENERIC_NAKAMOTO
  bool gen_env = false;  // its lockstep lanes: headers and block regions pooled in bk_lmem
  bool roll_fused = false;  // the last cpr_rollout_net(_env) ran as k_fc16_rollout_net
  bool is_ev = false;    // B_k or Tailstorm event-engine lanes
  // Nakamoto fused episodes: exact re-runs of flagged episodes on the event engine
  bool has_rerun = false;
  eth::EthParams NEP;    // the Ethereum lane in Nakamoto mode
  int64_t nak_bytes = 0;
  bool async_launch = false;  // last launch came from cpr_run_episodes_async
  std::shared_ptr<FuseTime> fuse_time;  // ... as a member of a fused group (else null)
  std::vector<uint8_t> table_host;
  DevBuf table_dev, tabs_dev;  // policy table; unit-observation tables
  DevBuf summary, records;
  DevBuf pol_obs, pol_act;  // cpr_policy_actions staging, reused across calls
  DevBuf tr_off, tr_miner, tr_delay, tr_pow, tr_key, tr_ldelay;  // cpr_replay trace copy
  // lockstep lanes
  DevBuf lanes, lring, lspill, lreplay, l_obs, l_act, l_rew, l_done, l_mask, l_eps, l_info;
  // exact Nakamoto lockstep lanes (LockBuffers): action log, event-engine slots
  DevBuf l_alog, l_emem, l_eslots, l_efree;
  int64_t alog_cap = 0;
  int32_t n_exact_slots = 0;
  // cpr_rollout over the closed-form lanes: per-lane step cursor; summary + lanes-left word
  DevBuf l_cur, l_rsum;
  // neural-network policy (cpr_policy_net_set): the weights in one device buffer and the
  // kernel's view of them; cpr_rollout_net's lane cursors (episode step index, activations
  // already counted, activations at the end); cpr_policy_net_forward staging
  bool has_net = false;
  PolNet pn;
  DevBuf pn_w, pn_step, pn_acts0, pn_acts, pn_in, pn_out;
  // lane env (cpr_lane_env_set): the alpha table as thresholds and values, and per lane the
  // current episode's threshold and alpha and the dense wrapper's accumulator
  bool has_env = false;
  cpr_lane_env env = {};  // n_alpha >= 1 once set (cfg.alpha alone without a table)
  bool env_table = false; // the caller gave a table: cpr_rollout is refused
  DevBuf le_tab_t, le_tab_a, le_lane_t, le_lane_a, le_acc;
  int32_t schedule = CPR_SCHEDULE_CHOICE;  // cpr_lane_env_schedule
  // cpr_eval_net: the set's records, per-lane episode reward, the finished-episode counter,
  // per-alpha summaries and statistics; `parked`: an evaluation left the lanes in arbitrary
  // later episodes, and stepping them waits for a reset of every lane
  DevBuf ev_rec, ev_acc, ev_cnt, ev_sum, ev_alpha;
  bool parked = false;
  // the learner (cpr_ppo_*): where each parameter array stands in pn_w (floats, arrays padded
  // to 4) and its length, in the flat gradient's order; Adam's moments and step count; the
  // number of updates since the network was set (the permutation's counter); per-minibatch
  // scratch; staging of host data; cpr_ppo_iterate's rollout buffers
  std::vector<int64_t> pn_off, pn_cnt;
  int64_t pn_total = 0;
  int64_t ppo_t = 0, ppo_updates = 0;
  DevBuf pp_m, pp_v, pp_grad, pp_part, pp_xin, pp_act, pp_dy0, pp_dy1, pp_dlg, pp_dv, pp_advn,
      pp_partial, pp_stats, pp_red, pp_bpart, pp_idx, pp_perm;
  DevBuf pp_obs, pp_alpha, pp_action, pp_logp, pp_adv, pp_ret;
  std::vector<int32_t> perm_host;
  DevBuf it_obs, it_alpha, it_action, it_reward, it_done, it_logp, it_value, it_adv, it_ret;
  // Q-learning (cpr_dqn_*): the replay ring of dq_cap slots (and a guard slot) of n_lanes
  // transitions as structure of arrays, its cursor and size in slots, the vector steps
  // collected and the updates run since cpr_dqn_init; the target network (dq_tn: pn over
  // dq_tw); the gradient (its vf part stays zero), the indices of the last update; staging of
  // cpr_dqn_gradients' host data
  bool dq_ready = false;
  int64_t dq_cap = 0, dq_cursor = 0, dq_size = 0, dq_steps = 0, dq_updates = 0;
  PolNet dq_tn;
  DevBuf dq_tw, dq_obs, dq_next, dq_alpha, dq_action, dq_reward, dq_done, dq_grad, dq_idx;
  int64_t dq_idx_n = 0;
  std::vector<int64_t> dq_idx_host;
  DevBuf ds_obs, ds_next, ds_alpha, ds_action, ds_reward, ds_done, ds_idx;
  bool reset_done = false;
  int32_t tab_n = 4096;
  hipEvent_t ev0 = nullptr, ev1 = nullptr;
  double last_ms = 0.0;
  int64_t last_acts = 0;
  int64_t last_lanes = 0, last_resident = 0;  // cpr_launch_shape
};

extern "C" {

const char* cpr_version(void) { return CPR_VERSION_STRING; }
int cpr_abi_version(void) { return CPR_ABI_VERSION; }
const char* cpr_last_error(void) { return g_err.c_str(); }

int cpr_device_count(int* out) {
  int n = 0;
  hipError_t e = hipGetDeviceCount(&n);
  if (e != hipSuccess) return fail(CPR_E_HIP, std::string("hipGetDeviceCount: ") + hipGetErrorString(e));
  *out = n;
  return CPR_OK;
}

static int flush_reruns(cpr_ctx* c);
// Launches the context's pending group of deferred cpr_run_episodes_async calls, if any. At
// the top of every entry point that takes a context or a batch (CPR_ENTER), so that whatever
// the entry does comes after the launches the caller has already asked for; an error of the
// deferred launch is returned by that entry
static int fuse_launch_pending(cpr_ctx* c);
#define CPR_ENTER(ctx_)                                             \
  do {                                                              \
    if (const int rc_ = fuse_launch_pending(ctx_)) return rc_;      \
  } while (0)

int cpr_ctx_create(int device, cpr_ctx** out) {
  if (!out) return fail(CPR_E_INVALID_ARG, "out is NULL");
  int n = 0;
  HIP_TRY(hipGetDeviceCount(&n));
  if (device < 0 || device >= n) return fail(CPR_E_INVALID_ARG, "no such HIP device");
  HIP_TRY(hipSetDevice(device));
  hipDeviceProp_t prop;
  HIP_TRY(hipGetDeviceProperties(&prop, device));
  cpr_ctx* c = new cpr_ctx;
  c->device = device;
  c->cus = prop.multiProcessorCount;
  hipError_t e = hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking);
  if (e == hipSuccess) e = hipStreamCreateWithFlags(&c->side, hipStreamNonBlocking);
  if (e == hipSuccess) e = hipEventCreateWithFlags(&c->main_ev, hipEventDisableTiming);
  for (int i = 0; i < 2 && e == hipSuccess; ++i)
    e = hipEventCreateWithFlags(&c->list_ev[i], hipEventDisableTiming);
  if (e != hipSuccess) {
    delete c;
    return fail(CPR_E_HIP, std::string("hipStreamCreate: ") + hipGetErrorString(e));
  }
  *out = c;
  return CPR_OK;
}

int cpr_ctx_destroy(cpr_ctx* c) {
  if (!c) return CPR_OK;
  (void)fuse_launch_pending(c);
  (void)hipSetDevice(c->device);
  // pending work first: queued exact re-runs complete their callers' summaries and records
  (void)flush_reruns(c);  // joins the side stream's second passes first
  (void)hipStreamSynchronize(c->stream);
  (void)hipStreamSynchronize(c->side);
  c->fl_free.insert(c->fl_free.end(), c->fl_pending.begin(), c->fl_pending.end());
  c->fl_pending.clear();
  for (cpr_ctx::FlushRec& r : c->fl_free) {
    (void)hipEventDestroy(r.e0);
    (void)hipEventDestroy(r.e1);
    (void)hipEventDestroy(r.e2);
    (void)hipHostFree(r.cnt);
  }
  (void)hipStreamDestroy(c->stream);
  (void)hipStreamDestroy(c->side);
  (void)hipEventDestroy(c->main_ev);
  for (int i = 0; i < 2; ++i) {
    (void)hipEventDestroy(c->list_ev[i]);
    c->lists[i].release();
  }
  c->rq.release();
  c->rtab.release();
  c->rmem.release();
  c->wq.release();
  delete c;
  return CPR_OK;
}

int cpr_synchronize(cpr_ctx* c) {
  CPR_ENTER(c);
  HIP_TRY(hipSetDevice(c->device));
  int rc = flush_reruns(c);  // joins the side stream first
  if (rc) return rc;
  HIP_TRY(hipStreamSynchronize(c->stream));
  return CPR_OK;
}

static uint64_t alpha_threshold(double alpha) {
  double t = alpha * 4294967296.0;
  if (t <= 0.0) return 0;
  if (t >= 4294967296.0) return 4294967296ull;
  return (uint64_t)t;
}

// engine.ml:37-51 and network.ml:61-76 (messages kept verbatim)
static int validate_eth(const cpr_config* c, eth::EthParams* P);

// the keyed miner draw for compute weights 1..n (models.ml:3-28), as the oracle's
// weight_thresholds: thr[i] = floor(sum_{j<=i} w_j / sum w * 2^32), i < n - 1
static void clique_thresholds(int n, uint32_t* thr) {
  double total = 0.0, cum = 0.0;
  for (int i = 0; i < n; ++i) total += (double)(i + 1);
  for (int i = 0; i + 1 < n; ++i) {
    cum += (double)(i + 1);
    const double t = cum / total * 4294967296.0;
    thr[i] = t <= 0.0 ? 0u : (t >= 4294967295.0 ? 4294967295u : (uint32_t)t);
  }
}

static int validate_bk(const cpr_config* c, bk::BkParams* P);
static int validate_ts(const cpr_config* c, ts::TsParams* P);

// Nakamoto configurations the closed-form lane does not cover run on the event engine:
// honest cliques; Simulator.loop tasks on the selfish-mining network at gamma = 0 (messages
// at t = +inf, drained after the last activation); and loop tasks whose message delays make
// overlapping windows common (the withholding sweep's 1e-4 defender delay overlaps about
// once per 10,000 activations, models.ml:54), which the closed-form lane would hand to
// the same engine episode by episode anyway
// the random attacker of the reference's policy tests (cpr_protocols.ml:658-782) decides in
// its handler: Simulator.loop tasks (the gym's agent takes actions from its caller)
static const char* random_policy_msg =
    "random attacker actions: Simulator.loop tasks (CPR_MODE_LOOP) on the event engines";

static bool nak_on_event_engine(const cpr_config* c) {
  if (c->protocol != CPR_PROTO_NAKAMOTO) return false;
  if (c->network == CPR_NET_HONEST_CLIQUE || c->network == CPR_NET_EXP_CLIQUE) return true;
  if (c->network != CPR_NET_SELFISH_MINING || c->mode != CPR_MODE_LOOP) return false;
  if (c->gamma == 0.0) return true;
  const double prop = c->propagation_delay > 0 ? c->propagation_delay : 1e-9;
  const double dd = (double)c->defenders;
  const double span = std::max(prop, (dd - 1.) / dd * prop / c->gamma);
  return !(span * (double)c->activations < 1e-3 * c->activation_delay);
}

// FC'16 abstract model (fc16.rs:141-158 FC16SSZwPT::new: Bernoulli(alpha), Bernoulli(gamma),
// Bernoulli(1 / horizon) reject probabilities outside [0, 1])
static int validate_fc16(const cpr_config* c, fc16::Fc16Params* P) {
  if (std::isnan(c->alpha) || c->alpha < 0. || c->alpha > 1.)
    return fail(CPR_E_INVALID_ARG, "alpha < 0 || alpha > 1");
  if (std::isnan(c->gamma) || c->gamma < 0. || c->gamma > 1.)
    return fail(CPR_E_INVALID_ARG, "gamma < 0 || gamma > 1");
  if (!(c->horizon >= 1.)) return fail(CPR_E_INVALID_ARG, "horizon must be >= 1");
  if (c->mode != CPR_MODE_GYM) return fail(CPR_E_UNSUPPORTED, "FC16 runs gym episodes");
  if (c->policy < CPR_FC16_POLICY_HONEST || c->policy > CPR_FC16_POLICY_TABLE)
    return fail(CPR_E_INVALID_ARG, "unknown policy");
  memset(P, 0, sizeof(*P));
  if (c->policy == CPR_FC16_POLICY_TABLE) {
    const int64_t D = c->policy_table_dim;
    if (!c->policy_table || D <= 0 || D > 256)
      return fail(CPR_E_INVALID_ARG, "policy table missing or dim out of range (1..256)");
    for (int64_t i = 0; i < D * D * 3; i++)
      if (c->policy_table[i] > 3) return fail(CPR_E_INVALID_ARG, "policy table action out of range");
    P->table_dim = (int32_t)D;
  }
  P->t_alpha = alpha_threshold(c->alpha);
  P->t_gamma = alpha_threshold(c->gamma);
  P->t_term = alpha_threshold(1.0 / c->horizon);
  P->max_steps = c->max_steps > 0 ? c->max_steps : (int64_t)1 << 30;
  P->policy = c->policy;
  return CPR_OK;
}

// The generic release/consider env over Nakamoto (gym/rust/src/generic/mod.rs:384-400 Env::new;
// generic_lane.h). max_steps bounds the lane's block DAG, so it is required.
static int validate_generic(const cpr_config* c, generic::GenericParams* P) {
  if (std::isnan(c->alpha) || c->alpha < 0. || c->alpha > 1.)
    return fail(CPR_E_INVALID_ARG, "alpha < 0 || alpha > 1");
  if (std::isnan(c->gamma) || c->gamma < 0. || c->gamma > 1.)
    return fail(CPR_E_INVALID_ARG, "gamma < 0 || gamma > 1");
  if (!(c->horizon >= 1.)) return fail(CPR_E_INVALID_ARG, "horizon must be >= 1");
  if (c->mode != CPR_MODE_GYM) return fail(CPR_E_UNSUPPORTED, "the generic env runs gym episodes");
  if (c->max_steps <= 0)
    return fail(CPR_E_INVALID_ARG, "generic env: max_steps must be > 0 (it bounds the lane's "
                                   "block DAG)");
  if (c->max_steps > generic::kGenericMaxSteps)
    return fail(CPR_E_INVALID_ARG, "generic env: max_steps above the built cap of " +
                                       std::to_string(generic::kGenericMaxSteps));
  if (c->k < 1 || c->k > generic::kGenericMaxK)
    return fail(CPR_E_INVALID_ARG, "generic env: k (release / consider entries of the "
                                   "network's action head) must be in 1..11");
  memset(P, 0, sizeof(*P));
  P->t_alpha = alpha_threshold(c->alpha);
  P->t_gamma = alpha_threshold(c->gamma);
  P->t_term = alpha_threshold(1.0 / c->horizon);
  P->max_steps = (int32_t)c->max_steps;
  return CPR_OK;
}

static int validate(const cpr_config* c, NakParams* P, eth::EthParams* EP, bk::BkParams* BP,
                    ts::TsParams* TP) {
  if (c->protocol == CPR_PROTO_ETHEREUM) return validate_eth(c, EP);
  if (c->protocol == CPR_PROTO_BK) return validate_bk(c, BP);
  if (c->protocol == CPR_PROTO_TAILSTORM) return validate_ts(c, TP);
  if (c->protocol != CPR_PROTO_NAKAMOTO)
    return fail(CPR_E_UNSUPPORTED, "protocol not implemented on the device yet");
  if (c->network == CPR_NET_HONEST_CLIQUE) {
    // every node honest: the event engine in Nakamoto mode (no closed form for cliques)
    cpr_config c2 = *c;
    c2.protocol = CPR_PROTO_ETHEREUM;
    c2.policy = CPR_ETH_POLICY_HONEST;
    c2.reward_scheme = CPR_REWARD_CONSTANT;
    const int rc = validate_eth(&c2, EP);
    if (rc) return rc;
    EP->nak = 1;
    return CPR_OK;
  }
  if (std::isnan(c->activation_delay)) return fail(CPR_E_INVALID_ARG, "activation_delay cannot be NaN");
  if (std::isnan(c->alpha)) return fail(CPR_E_INVALID_ARG, "alpha cannot be NaN");
  if (std::isnan(c->gamma)) return fail(CPR_E_INVALID_ARG, "gamma cannot be NaN");
  if (c->alpha < 0. || c->alpha > 1.) return fail(CPR_E_INVALID_ARG, "alpha < 0 || alpha > 1");
  if (c->gamma < 0. || c->gamma > 1.) return fail(CPR_E_INVALID_ARG, "gamma < 0 || gamma > 1");
  if (c->activation_delay <= 0.) return fail(CPR_E_INVALID_ARG, "activation_delay <= 0");
  if (c->mode != CPR_MODE_GYM && c->mode != CPR_MODE_LOOP)
    return fail(CPR_E_INVALID_ARG, "unknown mode");
  if (c->policy < CPR_POLICY_HONEST || c->policy > CPR_POLICY_RANDOM)
    return fail(CPR_E_INVALID_ARG, "unknown policy");
  if (c->policy == CPR_POLICY_RANDOM && !(c->mode == CPR_MODE_LOOP && nak_on_event_engine(c)))
    return fail(CPR_E_UNSUPPORTED, random_policy_msg);
  if (c->policy == CPR_POLICY_TABLE) {
    if (!c->policy_table || c->policy_table_dim <= 0 || c->policy_table_dim > 256)
      return fail(CPR_E_INVALID_ARG, "policy table missing or dim out of range (1..256)");
    for (int i = 0; i < c->policy_table_dim * c->policy_table_dim * 2; i++)
      if (c->policy_table[i] > 3) return fail(CPR_E_INVALID_ARG, "policy table action out of range");
  }
  if (nak_on_event_engine(c)) {
    // Simulator.loop on the selfish-mining network at gamma = 0: the attacker's messages
    // arrive at t = +inf and the loop drains them after the last activation
    // (simulator.ml:519-533); no closed form, so the event engine in Nakamoto mode runs it
    cpr_config c2 = *c;
    c2.protocol = CPR_PROTO_ETHEREUM;
    c2.policy = CPR_ETH_POLICY_HONEST;
    c2.reward_scheme = CPR_REWARD_CONSTANT;
    const int rc = validate_eth(&c2, EP);
    if (rc) return rc;
    EP->nak = 1;
    EP->policy = c->policy;
    EP->table_dim = c->policy_table_dim;
    return CPR_OK;
  }
  memset(P, 0, sizeof(*P));
  P->ev = c->activation_delay;
  P->t_att = alpha_threshold(c->alpha);
  P->policy = c->policy;
  P->table_dim = c->policy_table_dim;
  if (c->network == CPR_NET_SELFISH_MINING) {
    if (c->defenders < 1) return fail(CPR_E_INVALID_ARG, "defenders < 0");
    if (c->defenders < 2) return fail(CPR_E_INVALID_ARG, "defenders must be at least 2");
    if (c->defenders > 64)
      return fail(CPR_E_UNSUPPORTED, "device lanes support at most 64 defenders");
    const double dd = (double)c->defenders;
    if (c->gamma > (dd - 1.) / dd)
      return fail(CPR_E_INVALID_ARG, "gamma must not be greater ( (defenders - 1) / defenders )");
    const double prop = c->propagation_delay > 0 ? c->propagation_delay : 1e-9;
    P->d = c->defenders;
    P->delta = prop;
    P->dmax = (dd - 1.) / dd * prop / c->gamma;
    P->arrive = std::isfinite(P->dmax) ? 1 : 0;
  } else if (c->network == CPR_NET_TWO_AGENTS) {
    if (c->mode == CPR_MODE_GYM)
      return fail(CPR_E_UNSUPPORTED, "the gym engine always uses the selfish-mining network");
    P->d = 1;
    P->delta = 0.0;
    P->dmax = 0.0;
    P->arrive = 1;
  } else if (c->network == CPR_NET_ABSTRACT_GAMMA) {
    // flagged abstract-gamma mode (include/cpr_hip.h): zero delays, coin-decided races
    if (c->mode != CPR_MODE_GYM)
      return fail(CPR_E_UNSUPPORTED, "the abstract-gamma mode runs gym episodes");
    if (c->defenders < 1 || c->defenders > 64)
      return fail(CPR_E_INVALID_ARG, "abstract gamma: 1..64 defenders");
    P->d = c->defenders;
    P->delta = 0.0;
    P->dmax = 0.0;
    P->arrive = 1;
    P->abstract_g = 1;
    P->gamma = c->gamma;
  } else {
    return fail(CPR_E_INVALID_ARG, "unknown network");
  }
  int64_t span;  // activations per episode + 1 (bound on chain length and clock index)
  if (c->mode == CPR_MODE_GYM) {
    const int64_t ms = c->max_steps > 0 ? c->max_steps : INT64_MAX;
    P->max_steps = ms;
    P->max_progress = c->max_progress > 0 ? c->max_progress : __builtin_inf();
    P->max_time = c->max_time > 0 ? c->max_time : __builtin_inf();
    span = ms < (1 << 20) ? ms + 2 : 4096;
  } else {
    if (c->activations <= 0) return fail(CPR_E_INVALID_ARG, "activations <= 0");
    if (c->activations > (1 << 24)) return fail(CPR_E_UNSUPPORTED, "activations > 2^24");
    P->max_steps = INT64_MAX;
    P->max_progress = __builtin_inf();
    P->max_time = __builtin_inf();
    span = c->activations + 2;
  }
  P->cap = (int32_t)(((std::min<int64_t>(span, 1 << 20) + 63) / 64) * 64);
  return CPR_OK;
}

// Ethereum: engine.ml:37-51 checks shared with Nakamoto, network.ml:61-76, ethereum_ssz
// policies 0..4, Constant / Discount rewards
static int validate_eth(const cpr_config* c, eth::EthParams* P) {
  if (std::isnan(c->activation_delay)) return fail(CPR_E_INVALID_ARG, "activation_delay cannot be NaN");
  if (std::isnan(c->alpha)) return fail(CPR_E_INVALID_ARG, "alpha cannot be NaN");
  if (std::isnan(c->gamma)) return fail(CPR_E_INVALID_ARG, "gamma cannot be NaN");
  if (c->alpha < 0. || c->alpha > 1.) return fail(CPR_E_INVALID_ARG, "alpha < 0 || alpha > 1");
  if (c->gamma < 0. || c->gamma > 1.) return fail(CPR_E_INVALID_ARG, "gamma < 0 || gamma > 1");
  if (c->activation_delay <= 0.) return fail(CPR_E_INVALID_ARG, "activation_delay <= 0");
  if (c->mode != CPR_MODE_GYM && c->mode != CPR_MODE_LOOP)
    return fail(CPR_E_INVALID_ARG, "unknown mode");
  if (c->policy < CPR_ETH_POLICY_HONEST || c->policy > CPR_ETH_POLICY_RANDOM)
    return fail(CPR_E_INVALID_ARG, "unknown policy");
  if (c->policy == CPR_ETH_POLICY_RANDOM && c->mode != CPR_MODE_LOOP)
    return fail(CPR_E_UNSUPPORTED, random_policy_msg);
  if (c->reward_scheme != CPR_REWARD_CONSTANT && c->reward_scheme != CPR_REWARD_DISCOUNT)
    return fail(CPR_E_INVALID_ARG, "unknown incentive scheme");
  if (c->policy == CPR_ETH_POLICY_TABLE) {
    const int64_t D = c->policy_table_dim;
    if (!c->policy_table || D <= 0 || D > 64)
      return fail(CPR_E_INVALID_ARG, "policy table missing or dim out of range (1..64)");
    for (int64_t i = 0; i < D * D * 2; i++)
      if (c->policy_table[i] > 23) return fail(CPR_E_INVALID_ARG, "policy table action out of range");
  }
  memset(P, 0, sizeof(*P));
  P->table_dim = c->policy == CPR_ETH_POLICY_TABLE ? c->policy_table_dim : 0;
  P->ev = c->activation_delay;
  P->t_att = alpha_threshold(c->alpha);
  P->policy = c->policy;
  P->scheme = c->reward_scheme;
  P->mode = c->mode;
  if (c->network == CPR_NET_SELFISH_MINING) {
    if (c->defenders < 1) return fail(CPR_E_INVALID_ARG, "defenders < 0");
    if (c->defenders < 2) return fail(CPR_E_INVALID_ARG, "defenders must be at least 2");
    if (c->defenders > 64)
      return fail(CPR_E_UNSUPPORTED, "device lanes support at most 64 defenders");
    const double dd = (double)c->defenders;
    if (c->gamma > (dd - 1.) / dd)
      return fail(CPR_E_INVALID_ARG, "gamma must not be greater ( (defenders - 1) / defenders )");
    const double prop = c->propagation_delay > 0 ? c->propagation_delay : 1e-9;
    P->d = c->defenders;
    P->net = 0;
    P->delta = prop;
    P->dmax = (dd - 1.) / dd * prop / c->gamma;
  } else if (c->network == CPR_NET_TWO_AGENTS) {
    if (c->mode == CPR_MODE_GYM)
      return fail(CPR_E_UNSUPPORTED, "the gym engine always uses the selfish-mining network");
    P->d = 1;
    P->net = 1;
  } else if (c->network == CPR_NET_HONEST_CLIQUE) {
    // models.ml:3-28: n honest nodes with compute i + 1, uniform link delays
    if (c->mode != CPR_MODE_LOOP)
      return fail(CPR_E_UNSUPPORTED, "honest cliques run Simulator.loop tasks (CPR_MODE_LOOP)");
    if (c->defenders < 2 || c->defenders > 64)
      return fail(CPR_E_INVALID_ARG, "honest clique: 2..64 nodes (cfg.defenders)");
    const bool dflt = std::isnan(c->delay_lo) && std::isnan(c->delay_hi);  // NaN: models.ml default
    const double lo = dflt ? 0.5 : c->delay_lo, hi = dflt ? 1.5 : c->delay_hi;
    if (!(lo >= 0.) || !(hi >= lo)) return fail(CPR_E_INVALID_ARG, "delay_lo/delay_hi");
    P->d = c->defenders - 1;
    P->net = 2;
    P->lo = lo;
    P->hi = hi;
    clique_thresholds(c->defenders, P->thr);
  } else if (c->network == CPR_NET_EXP_CLIQUE) {
    // cpr_protocols.ml:478-485: symmetric clique, exponential link delays, node 0 runs the
    // attack policy (ethereum_ssz, or nakamoto_ssz in Nakamoto mode); keyed equal-weight
    // miner draw (attacker threshold 1/n)
    if (c->mode != CPR_MODE_LOOP)
      return fail(CPR_E_UNSUPPORTED, "the gym engine always uses the selfish-mining network");
    if (c->defenders < 1 || c->defenders > 63)
      return fail(CPR_E_INVALID_ARG, "exponential clique: 1..63 defenders");
    if (!(c->propagation_delay > 0.) || !std::isfinite(c->propagation_delay))
      return fail(CPR_E_INVALID_ARG, "exponential clique: propagation_delay must be positive");
    P->d = c->defenders;
    P->net = 3;
    P->delta = c->propagation_delay;
    P->t_att = alpha_threshold(1.0 / (double)(c->defenders + 1));
  } else {
    return fail(CPR_E_INVALID_ARG, "unknown network");
  }
  P->n = P->d + 1;
  int64_t span;
  if (c->mode == CPR_MODE_GYM) {
    const int64_t ms = c->max_steps > 0 ? c->max_steps : INT64_MAX;
    P->max_steps = ms;
    P->max_progress = c->max_progress > 0 ? c->max_progress : __builtin_inf();
    P->max_time = c->max_time > 0 ? c->max_time : __builtin_inf();
    span = ms < (1 << 20) ? ms + 2 : 4096;
  } else {
    if (c->activations <= 0) return fail(CPR_E_INVALID_ARG, "activations <= 0");
    if (c->activations > (1 << 24)) return fail(CPR_E_UNSUPPORTED, "activations > 2^24");
    P->max_steps = INT64_MAX;
    P->activations = c->activations;
    P->max_progress = __builtin_inf();
    P->max_time = __builtin_inf();
    span = c->activations + 2;
  }
  // the block ring holds a whole episode up to 2^15 blocks (longer episodes flag
  // CPR_ST_CAPACITY only if a fork outlives the ring); heap: 512 in-flight events per node
  int32_t cb = 64;
  while (cb < span && cb < (1 << 15)) cb <<= 1;
  P->cap_b = cb;
  // gamma = 0: messages at t = +inf stay in the skew heap (they shape its tie order);
  // otherwise an attacker release shares every withheld block at once, d messages each
  // (a 300-block release at alpha .45, gamma .9 overflowed 512 events per node), and each
  // block is released at most once: d messages per block of the episode bound the heap
  int64_t extra = 0;
  const int64_t ext = P->mode == CPR_MODE_LOOP ? span : std::min<int64_t>(span, 8192);
  if (P->net == 0 && !std::isfinite(P->dmax))
    extra = 2 * (int64_t)P->d * ext;
  else if (P->net == 0 || P->net == 3)
    extra = (int64_t)P->d * ext;
  P->cap_e = 64 + 512 * P->n + (int32_t)std::min<int64_t>(extra, 1 << 24);
  return CPR_OK;
}

// vertex-ring window of the B_k / Tailstorm lanes (see validate_bk)
static constexpr int32_t kRingWindow = 4096;
// HBM budget for the per-lane regions of the event-engine lanes (288 GB per MI355X)
static constexpr int64_t kLaneBudget = 96ll << 30;

// B_k: engine.ml:37-51 checks shared with Nakamoto, network.ml:61-76, bk.ml k >= 1,
// Constant / Block rewards, bk_ssz policies 0..3 or a table
static int validate_bk(const cpr_config* c, bk::BkParams* P) {
  if (std::isnan(c->activation_delay)) return fail(CPR_E_INVALID_ARG, "activation_delay cannot be NaN");
  if (std::isnan(c->alpha)) return fail(CPR_E_INVALID_ARG, "alpha cannot be NaN");
  if (std::isnan(c->gamma)) return fail(CPR_E_INVALID_ARG, "gamma cannot be NaN");
  if (c->alpha < 0. || c->alpha > 1.) return fail(CPR_E_INVALID_ARG, "alpha < 0 || alpha > 1");
  if (c->gamma < 0. || c->gamma > 1.) return fail(CPR_E_INVALID_ARG, "gamma < 0 || gamma > 1");
  if (c->activation_delay <= 0.) return fail(CPR_E_INVALID_ARG, "activation_delay <= 0");
  if (c->mode != CPR_MODE_GYM && c->mode != CPR_MODE_LOOP)
    return fail(CPR_E_INVALID_ARG, "unknown mode");
  if (c->k < 1) return fail(CPR_E_INVALID_ARG, "k must be positive");
  if (c->k > 64) return fail(CPR_E_UNSUPPORTED, "device lanes support k <= 64");
  if (c->reward_scheme != CPR_REWARD_CONSTANT && c->reward_scheme != CPR_REWARD_BLOCK)
    return fail(CPR_E_INVALID_ARG, "'" + std::to_string(c->reward_scheme) +
                                       "' is not a valid parameter choice, try 'block' or 'constant'");
  if (c->policy < CPR_BK_POLICY_HONEST || c->policy > CPR_BK_POLICY_RANDOM)
    return fail(CPR_E_INVALID_ARG, "unknown policy");
  if (c->policy == CPR_BK_POLICY_RANDOM && c->mode != CPR_MODE_LOOP)
    return fail(CPR_E_UNSUPPORTED, random_policy_msg);
  memset(P, 0, sizeof(*P));
  if (c->policy == CPR_BK_POLICY_TABLE) {
    const int64_t D = c->policy_table_dim;
    if (!c->policy_table || D <= 0 || D > 64)
      return fail(CPR_E_INVALID_ARG, "policy table missing or dim out of range (1..64)");
    const int64_t sz = D * D * (c->k + 1) * (c->k + 1) * 3;
    for (int64_t i = 0; i < sz; i++)
      if (c->policy_table[i] > 7) return fail(CPR_E_INVALID_ARG, "policy table action out of range");
    P->table_dim = (int32_t)D;
  }
  P->ev = c->activation_delay;
  P->t_att = alpha_threshold(c->alpha);
  P->policy = c->policy;
  P->scheme = c->reward_scheme;
  P->mode = c->mode;
  P->k = c->k;
  if (c->network == CPR_NET_SELFISH_MINING) {
    if (c->defenders < 1) return fail(CPR_E_INVALID_ARG, "defenders < 0");
    if (c->defenders < 2) return fail(CPR_E_INVALID_ARG, "defenders must be at least 2");
    if (c->defenders > 64)
      return fail(CPR_E_UNSUPPORTED, "device lanes support at most 64 defenders");
    const double dd = (double)c->defenders;
    if (c->gamma > (dd - 1.) / dd)
      return fail(CPR_E_INVALID_ARG, "gamma must not be greater ( (defenders - 1) / defenders )");
    const double prop = c->propagation_delay > 0 ? c->propagation_delay : 1e-9;
    P->d = c->defenders;
    P->net = 0;
    P->delta = prop;
    P->dmax = (dd - 1.) / dd * prop / c->gamma;
  } else if (c->network == CPR_NET_TWO_AGENTS) {
    if (c->mode == CPR_MODE_GYM)
      return fail(CPR_E_UNSUPPORTED, "the gym engine always uses the selfish-mining network");
    P->d = 1;
    P->net = 1;
  } else if (c->network == CPR_NET_HONEST_CLIQUE) {
    // models.ml:3-28: n honest nodes with compute i + 1, uniform link delays; node 0 runs
    // the honest protocol too (the policy is ignored)
    if (c->mode != CPR_MODE_LOOP)
      return fail(CPR_E_UNSUPPORTED, "honest cliques run Simulator.loop tasks (CPR_MODE_LOOP)");
    if (c->defenders < 2 || c->defenders > 64)
      return fail(CPR_E_INVALID_ARG, "honest clique: 2..64 nodes (cfg.defenders)");
    const bool dflt = std::isnan(c->delay_lo) && std::isnan(c->delay_hi);  // NaN: models.ml default
    const double lo = dflt ? 0.5 : c->delay_lo, hi = dflt ? 1.5 : c->delay_hi;
    if (!(lo >= 0.) || !(hi >= lo)) return fail(CPR_E_INVALID_ARG, "delay_lo/delay_hi");
    P->d = c->defenders - 1;
    P->net = 2;
    P->lo = lo;
    P->hi = hi;
    clique_thresholds(c->defenders, P->thr);
  } else if (c->network == CPR_NET_EXP_CLIQUE) {
    // cpr_protocols.ml:478-485: symmetric clique, exponential link delays, node 0 runs the
    // attack policy; the oracle's keyed draw for equal compute 1/n (attacker threshold)
    if (c->mode != CPR_MODE_LOOP)
      return fail(CPR_E_UNSUPPORTED, "the gym engine always uses the selfish-mining network");
    if (c->defenders < 1 || c->defenders > 63)
      return fail(CPR_E_INVALID_ARG, "exponential clique: 1..63 defenders");
    if (!(c->propagation_delay > 0.) || !std::isfinite(c->propagation_delay))
      return fail(CPR_E_INVALID_ARG, "exponential clique: propagation_delay must be positive");
    P->d = c->defenders;
    P->net = 3;
    P->delta = c->propagation_delay;
    P->t_att = alpha_threshold(1.0 / (double)(c->defenders + 1));
  } else {
    return fail(CPR_E_INVALID_ARG, "unknown network");
  }
  P->n = P->d + 1;
  int64_t span;
  if (c->mode == CPR_MODE_GYM) {
    const int64_t ms = c->max_steps > 0 ? c->max_steps : INT64_MAX;
    P->max_steps = ms;
    P->max_progress = c->max_progress > 0 ? c->max_progress : __builtin_inf();
    P->max_time = c->max_time > 0 ? c->max_time : __builtin_inf();
    span = ms < (1 << 20) ? ms + 2 : 8192;
  } else {
    if (c->activations <= 0) return fail(CPR_E_INVALID_ARG, "activations <= 0");
    if (c->activations > (1 << 24)) return fail(CPR_E_UNSUPPORTED, "activations > 2^24");
    P->max_steps = INT64_MAX;
    P->activations = c->activations;
    P->max_progress = __builtin_inf();
    P->max_time = __builtin_inf();
    span = c->activations * 2 + 2;  // votes + blocks
  }
  // vertex ring: a window of at most 4096 vertices (a whole 2048-step gym episode); longer
  // runs flag CPR_ST_CAPACITY only if something older than the window is read (a fork
  // that outlives it). Small per-lane regions let the grid reach resident capacity.
  int32_t cv = 64;
  while (cv < span + 64 && cv < kRingWindow) cv <<= 1;
  P->cap_v = cv;
  P->cap_q = cv / 2;
  P->cap_d = 64;
  P->cap_e = 256 + 512 * P->n +
             (std::isfinite(P->dmax) || P->net == 1
                  ? 0
                  : (int32_t)(2 * P->d * std::min<int64_t>(span, 8192)));
  return CPR_OK;
}

// Tailstorm: engine.ml:37-51 checks, network.ml:61-76, tailstorm.ml k >= 1, the four
// incentive schemes and three sub-block selections, tailstorm_ssz policies 0..6
static int validate_ts(const cpr_config* c, ts::TsParams* P) {
  // the B_k checks cover everything but the scheme, selection and policy ranges
  cpr_config cb = *c;
  cb.protocol = CPR_PROTO_BK;
  cb.reward_scheme = CPR_REWARD_CONSTANT;
  cb.policy = CPR_BK_POLICY_HONEST;
  bk::BkParams B;
  int rc = validate_bk(&cb, &B);
  if (rc) return rc;
  if (c->reward_scheme != CPR_REWARD_CONSTANT && c->reward_scheme != CPR_REWARD_DISCOUNT &&
      c->reward_scheme != CPR_REWARD_PUNISH && c->reward_scheme != CPR_REWARD_HYBRID)
    return fail(CPR_E_INVALID_ARG, "'" + std::to_string(c->reward_scheme) +
                                       "' is not a valid parameter choice, try 'constant', "
                                       "'discount', 'punish' or 'hybrid'");
  if (c->subblock_selection < CPR_SELECT_ALTRUISTIC || c->subblock_selection > CPR_SELECT_OPTIMAL)
    return fail(CPR_E_INVALID_ARG, "'" + std::to_string(c->subblock_selection) +
                                       "' is not a valid parameter choice, try 'altruistic', "
                                       "'heuristic' or 'optimal'");
  if (c->policy < CPR_TS_POLICY_HONEST || c->policy > CPR_TS_POLICY_RANDOM)
    return fail(CPR_E_INVALID_ARG, "unknown policy");
  if (c->policy == CPR_TS_POLICY_RANDOM && c->mode != CPR_MODE_LOOP)
    return fail(CPR_E_UNSUPPORTED, random_policy_msg);
  if (c->policy == CPR_TS_POLICY_TABLE) {
    const int64_t D = c->policy_table_dim;
    if (!c->policy_table || D <= 0 || D > 64)
      return fail(CPR_E_INVALID_ARG, "policy table missing or dim out of range (1..64)");
    const int64_t sz = D * D * (c->k + 1) * (c->k + 1) * 3;
    for (int64_t i = 0; i < sz; i++)
      if (c->policy_table[i] > 7) return fail(CPR_E_INVALID_ARG, "policy table action out of range");
  }
  memset(P, 0, sizeof(*P));
  P->opt_budget = ts::TS_OPT_BUDGET;
  P->table_dim = c->policy == CPR_TS_POLICY_TABLE ? c->policy_table_dim : 0;
  P->t_att = B.t_att;
  P->d = B.d;
  P->n = B.n;
  P->net = B.net;
  P->mode = B.mode;
  P->policy = c->policy;
  P->scheme = c->reward_scheme;
  P->selection = c->subblock_selection;
  P->k = c->k;
  P->ev = B.ev;
  P->delta = B.delta;
  P->dmax = B.dmax;
  P->max_steps = B.max_steps;
  P->activations = B.activations;
  P->max_progress = B.max_progress;
  P->max_time = B.max_time;
  P->lo = B.lo;
  P->hi = B.hi;
  memcpy(P->thr, B.thr, sizeof(P->thr));
  // gym: one vertex per attacker interaction plus summaries; loop: ~ (1 + 1/k) per
  // activation. Vertex ring covers the whole episode up to 2^16 vertices.
  const int64_t span = c->mode == CPR_MODE_GYM
                           ? (B.max_steps < (1 << 20) ? B.max_steps + 2 : 8192)
                           : c->activations * 2 + 2;
  int32_t cv = 64;
  while (cv < span + 64 && cv < kRingWindow) cv <<= 1;
  P->cap_v = cv;
  P->cap_q = cv / 2;
  P->cap_d = 64;
  P->cap_e = 256 + 512 * P->n +
             (std::isfinite(P->dmax) || P->net == 1
                  ? 0
                  : (int32_t)(2 * P->d * std::min<int64_t>(span, 8192)));
  return CPR_OK;
}

int cpr_batch_create(cpr_ctx* ctx, const cpr_config* cfg, cpr_batch** out) {
  if (!ctx || !cfg || !out) return fail(CPR_E_INVALID_ARG, "NULL argument");
  CPR_ENTER(ctx);
  NakParams P;
  eth::EthParams EP;
  bk::BkParams BP;
  ts::TsParams TP;
  memset(&P, 0, sizeof(P));
  memset(&EP, 0, sizeof(EP));
  memset(&BP, 0, sizeof(BP));
  memset(&TP, 0, sizeof(TP));
  fc16::Fc16Params FP;
  memset(&FP, 0, sizeof(FP));
  const bool is_fc16 = cfg->protocol == CPR_PROTO_FC16 || cfg->protocol == CPR_PROTO_FC16_ENV;
  generic::GenericParams GP;
  memset(&GP, 0, sizeof(GP));
  const bool gen_env = cfg->protocol == CPR_PROTO_GENERIC_NAKAMOTO;
  int rc = gen_env   ? validate_generic(cfg, &GP)
           : is_fc16 ? validate_fc16(cfg, &FP)
                     : validate(cfg, &P, &EP, &BP, &TP);
  if (rc) return rc;
  HIP_TRY(hipSetDevice(ctx->device));
  cpr_batch* b = new cpr_batch;
  b->ctx = ctx;
  b->cfg = *cfg;
  b->P = P;
  b->EP = EP;
  b->BP = BP;
  b->TP = TP;
  b->FP = FP;
  b->is_fc16 = is_fc16;
  b->fc16_env = cfg->protocol == CPR_PROTO_FC16_ENV;
  b->GP = GP;
  b->gen_env = gen_env;
  b->eth_bytes = eth::eth_lane_bytes(EP.cap_b, EP.cap_e, EP.n);
  if (cfg->protocol == CPR_PROTO_BK) b->bk_bytes = bk::bk_lane_bytes(BP);
  if (cfg->protocol == CPR_PROTO_TAILSTORM) b->bk_bytes = ts::ts_lane_bytes(TP);
  b->is_ev = cfg->protocol == CPR_PROTO_BK || cfg->protocol == CPR_PROTO_TAILSTORM;
  b->is_eth = cfg->protocol == CPR_PROTO_ETHEREUM;
  b->nak_ev = nak_on_event_engine(cfg);
  b->cfg.policy_table = nullptr;
  if (cfg->protocol == CPR_PROTO_BK && cfg->policy == CPR_BK_POLICY_TABLE) {
    const size_t D = (size_t)cfg->policy_table_dim, K1 = (size_t)cfg->k + 1;
    b->table_host.assign(cfg->policy_table, cfg->policy_table + D * D * K1 * K1 * 3);
  } else if ((cfg->protocol == CPR_PROTO_NAKAMOTO && cfg->policy == CPR_POLICY_TABLE) ||
             (cfg->protocol == CPR_PROTO_ETHEREUM && cfg->policy == CPR_ETH_POLICY_TABLE)) {
    const size_t nb = (size_t)cfg->policy_table_dim * cfg->policy_table_dim * 2;
    b->table_host.assign(cfg->policy_table, cfg->policy_table + nb);
  } else if (is_fc16 && cfg->policy == CPR_FC16_POLICY_TABLE) {
    const size_t D = (size_t)cfg->policy_table_dim;
    b->table_host.assign(cfg->policy_table, cfg->policy_table + D * D * 3);
  } else if (cfg->protocol == CPR_PROTO_TAILSTORM && cfg->policy == CPR_TS_POLICY_TABLE) {
    const size_t D = (size_t)cfg->policy_table_dim, K1 = (size_t)cfg->k + 1;
    b->table_host.assign(cfg->policy_table, cfg->policy_table + D * D * K1 * K1 * 3);
  }
  // unit-observation tables (ssz_tools.ml:36-39) evaluated with the host libm:
  // [2/pi atan(i) | 0.5 + atan(i - N)/pi (2N) | 2/pi atan(i/k)], i < N
  const double kscale =
      (cfg->protocol == CPR_PROTO_BK || cfg->protocol == CPR_PROTO_TAILSTORM) ? (double)cfg->k : 1.0;
  std::vector<double> tabs(4 * (size_t)b->tab_n);
  for (int i = 0; i < b->tab_n; i++) tabs[i] = 2. / M_PI * std::atan((double)i / 1.0);
  for (int i = 0; i < 2 * b->tab_n; i++)
    tabs[b->tab_n + i] = 0.5 + (1. / M_PI * std::atan((double)(i - b->tab_n) / 1.0));
  for (int i = 0; i < b->tab_n; i++)
    tabs[3 * b->tab_n + i] = 2. / M_PI * std::atan((double)i / kscale);
  hipError_t e = b->tabs_dev.ensure(tabs.size() * sizeof(double));
  if (e == hipSuccess)
    e = hipMemcpy(b->tabs_dev.p, tabs.data(), tabs.size() * sizeof(double), hipMemcpyHostToDevice);
  if (e == hipSuccess && !b->table_host.empty()) {
    e = b->table_dev.ensure(b->table_host.size());
    if (e == hipSuccess)
      e = hipMemcpy(b->table_dev.p, b->table_host.data(), b->table_host.size(),
                    hipMemcpyHostToDevice);
  }
  if (e != hipSuccess) {
    delete b;
    return fail(CPR_E_HIP, std::string("batch buffers: ") + hipGetErrorString(e));
  }
  b->P.table = (const uint8_t*)b->table_dev.p;
  b->BP.table = (const uint8_t*)b->table_dev.p;
  b->EP.table = (const uint8_t*)b->table_dev.p;  // Nakamoto-mode or ethereum_ssz table
  b->TP.table = (const uint8_t*)b->table_dev.p;
  b->FP.table = (const uint8_t*)b->table_dev.p;
  if (cfg->protocol == CPR_PROTO_NAKAMOTO && !b->nak_ev) {
    // the same episode on the exact event engine: Ethereum lane, no uncles, nakamoto_ssz
    // policy (validated above); configurations it cannot hold keep the lane's flags
    cpr_config c2 = *cfg;
    c2.protocol = CPR_PROTO_ETHEREUM;
    c2.policy = CPR_ETH_POLICY_HONEST;
    c2.reward_scheme = CPR_REWARD_CONSTANT;
    const std::string keep_err = g_err;
    if (validate_eth(&c2, &b->NEP) == CPR_OK) {
      b->NEP.nak = 1;
      b->NEP.policy = cfg->policy;
      b->NEP.table = b->P.table;
      b->NEP.table_dim = cfg->policy_table_dim;
      b->nak_bytes = eth::eth_lane_bytes(b->NEP.cap_b, b->NEP.cap_e, b->NEP.n);
      b->has_rerun = true;
    }
    g_err = keep_err;
  }
  *out = b;
  return CPR_OK;
}

// lanes the device holds at once for this batch's fused-episode kernel (before any launch)
static int64_t batch_resident(cpr_batch* b) {
  const int64_t cus = b->ctx->cus;
  if (b->is_fc16) return cus * 8 * 256;
  if (b->cfg.protocol == CPR_PROTO_ETHEREUM || b->nak_ev) return cus * eth_blocks_per_cu() * 256;
  if (b->is_ev)
    return cus * (b->cfg.protocol == CPR_PROTO_TAILSTORM ? ts_blocks_per_cu() : bk_blocks_per_cu()) *
           256;
  return cus * run_episodes_blocks_per_cu(b->P, b->cfg.mode, false) * 256;
}

int cpr_launch_shape(cpr_batch* b, int64_t* lanes, int64_t* resident) {
  if (!b) return fail(CPR_E_INVALID_ARG, "NULL argument");
  CPR_ENTER(b->ctx);
  HIP_TRY(hipSetDevice(b->ctx->device));
  if (lanes) *lanes = b->last_lanes;
  if (resident) *resident = b->last_lanes ? b->last_resident : batch_resident(b);
  return CPR_OK;
}

int cpr_rerun_hbm_retries(cpr_ctx* c, int64_t* retries) {
  if (!c || !retries) return fail(CPR_E_INVALID_ARG, "NULL argument");
  CPR_ENTER(c);
  *retries = 0;
  if (!c->rq.p) return CPR_OK;
  HIP_TRY(hipSetDevice(c->device));
  HIP_TRY(side_join(c));
  uint32_t v = 0;
  HIP_TRY(hipStreamSynchronize(c->stream));
  HIP_TRY(hipMemcpy(&v, (char*)c->rq.p + (size_t)kRerunQueue * 8 + 4, 4, hipMemcpyDeviceToHost));
  *retries = v;
  return CPR_OK;
}

// fold finished flush records (oldest first: one stream, so they finish in order) into the
// totals and recycle them; wait: every one (cpr_rerun_stats), else only those done, plus the
// oldest while more than kFlushRecMax are outstanding
constexpr size_t kFlushRecMax = 32;

static int drain_flush_recs(cpr_ctx* c, bool wait) {
  while (!c->fl_pending.empty()) {
    const cpr_ctx::FlushRec r = c->fl_pending.front();
    if (wait || c->fl_pending.size() > kFlushRecMax) {
      HIP_TRY(hipEventSynchronize(r.e2));
    } else {
      const hipError_t q = hipEventQuery(r.e2);
      if (q == hipErrorNotReady) break;
      HIP_TRY(q);
    }
    float t = 0.f;
    HIP_TRY(hipEventElapsedTime(&t, r.e0, r.e1));
    c->rr_ms += t;
    c->rr_episodes += *r.cnt;
    c->rr_flushes += 1;
    c->fl_free.push_back(r);
    c->fl_pending.pop_front();
  }
  return CPR_OK;
}

int cpr_rerun_stats(cpr_ctx* c, int64_t* episodes, int64_t* flushes, double* ms) {
  if (!c) return fail(CPR_E_INVALID_ARG, "NULL argument");
  CPR_ENTER(c);
  HIP_TRY(hipSetDevice(c->device));
  if (const int rc = drain_flush_recs(c, true)) return rc;
  if (episodes) *episodes = c->rr_episodes;
  if (flushes) *flushes = c->rr_flushes;
  if (ms) *ms = c->rr_ms;
  return CPR_OK;
}

int cpr_lockstep_coverage(cpr_batch* b, int64_t* log_steps, int64_t* exact_slots) {
  if (!b) return fail(CPR_E_INVALID_ARG, "NULL argument");
  CPR_ENTER(b->ctx);
  if (log_steps) *log_steps = b->l_alog.p ? b->alog_cap : 0;
  if (exact_slots) *exact_slots = b->l_alog.p ? b->n_exact_slots : 0;
  return CPR_OK;
}

int cpr_last_launch(cpr_batch* b, double* kernel_ms, int64_t* activations) {
  if (!b) return fail(CPR_E_INVALID_ARG, "NULL argument");
  CPR_ENTER(b->ctx);
  if (b->async_launch) {  // cpr_run_episodes_async: waits for the end of that launch
    float ms = 0.f;
    if (b->fuse_time) {
      // a member of a fused group: its share of the group's kernel
      HIP_TRY(hipEventSynchronize(b->fuse_time->ev1));
      HIP_TRY(hipEventElapsedTime(&ms, b->fuse_time->ev0, b->fuse_time->ev1));
      ms /= (float)b->fuse_time->size;
      b->fuse_time.reset();
    } else {
      HIP_TRY(hipEventSynchronize(b->ev1));
      HIP_TRY(hipEventElapsedTime(&ms, b->ev0, b->ev1));
    }
    b->last_ms = ms;
    b->last_acts = -1;  // not known without reading the caller's device summary
    b->async_launch = false;
  }
  if (kernel_ms) *kernel_ms = b->last_ms;
  if (activations) *activations = b->last_acts;
  return CPR_OK;
}

int cpr_batch_destroy(cpr_batch* b) {
  if (!b) return CPR_OK;
  (void)fuse_launch_pending(b->ctx);  // this batch may be a member
  (void)hipSetDevice(b->ctx->device);
  (void)hipStreamSynchronize(b->ctx->stream);
  (void)flush_reruns(b->ctx);  // pending re-runs may read this batch's buffers
  (void)hipStreamSynchronize(b->ctx->stream);
  if (b->ev0) (void)hipEventDestroy(b->ev0);
  if (b->ev1) (void)hipEventDestroy(b->ev1);
  b->bk_lmem.release();
  b->bk_slots.release();
  for (DevBuf* d : {&b->table_dev, &b->tabs_dev, &b->summary,
                    &b->records, &b->lanes, &b->lring, &b->lspill, &b->lreplay,
                    &b->l_obs, &b->l_act, &b->l_rew, &b->l_done, &b->l_mask, &b->l_eps,
                    &b->l_info, &b->l_alog, &b->l_emem, &b->l_eslots, &b->l_efree, &b->l_cur,
                    &b->l_rsum, &b->tr_off, &b->tr_miner, &b->tr_delay, &b->tr_pow,
                    &b->tr_key, &b->tr_ldelay})
    d->release();
  delete b;
  return CPR_OK;
}

// lanes per launch: exactly the resident capacity (occupancy API: workgroups per CU at
// this kernel's register/LDS use x CUs x 256), bounded by a 16 GiB budget for per-lane HBM
// exact Nakamoto re-runs: one-wave workgroups of the re-run kernel
constexpr int64_t kRerunLanes = 512;
constexpr int64_t kRerunLanesMax = 8192;  // one workgroup per queued episode, up to this

// blocks_per_cu: of the kernel the launch runs
static int64_t episode_lanes(cpr_batch* b, int64_t n_eps, int blocks_per_cu) {
  const int64_t full = (int64_t)b->ctx->cus * blocks_per_cu * 256;
  const int64_t budget = (int64_t)(16ll << 30) / episode_lane_bytes(b->P);
  int64_t lanes = std::min(full, std::max<int64_t>(256, budget));
  // A/B: a share of the resident grid (percent), e.g. for launches that run concurrently
  if (const char* v = getenv("CPR_GRID_SCALE")) {
    const int64_t pc = atoll(v);
    if (pc > 0 && pc < 100) lanes = lanes * pc / 100;
  }
  lanes = std::max<int64_t>(256, (lanes / 256) * 256);
  // equal rounds: the episodes of a launch spread evenly over the fewest rounds of the
  // resident grid, so the last round is not a partly empty one (every lane's episode has
  // the same trip count in the gym)
  const int64_t rounds = std::max<int64_t>(1, (n_eps + lanes - 1) / lanes);
  const int64_t even = ((n_eps + rounds - 1) / rounds + 255) / 256 * 256;
  return std::max<int64_t>(256, std::min(lanes, even));
}

// Re-run every queued flagged Nakamoto episode of the launches since the last flush, in
// one k_nak_exact_rerun launch on the context's stream (after those launches, before the
// caller reads summaries or records), then empty the queue.
constexpr size_t kOvfMaxChunks = 4;  // overflow-flag chunks (256 MiB each) before a flush

static int flush_reruns(cpr_ctx* c) {
  // the side stream's second passes append to the queue and add to summaries: everything
  // after this point on the stream (the re-runs, the caller's reads) comes after them
  HIP_TRY(side_join(c));
  if (c->rlaunch.empty()) return CPR_OK;
  int64_t lb = 0, rest = 0;
  for (const RerunLaunch& r : c->rlaunch) {
    // the re-run region's layout (rerun_episode): the engine lane, then a hybrid's
    // closed-form ring, spill and tie-replay scratch (hybrid_mem); a launch registered with
    // a smaller region is refused here rather than run past it
    const int64_t need = eth::eth_lane_bytes(r.P.cap_b, r.P.cap_e, r.P.n) +
                         (r.hybrid ? hybrid_bytes(r.NP.cap) : 0);
    if (r.lane_bytes < need || (r.hybrid && r.NP.cap < r.P.max_steps + 2))
      return fail(CPR_E_HIP, "re-run region smaller than its layout (" +
                                 std::to_string(r.lane_bytes) + " < " + std::to_string(need) +
                                 " bytes)");
    lb = std::max(lb, r.lane_bytes);
    rest = std::max(rest, eth::eth_rest_bytes(r.P.cap_b, r.P.cap_e, r.P.n));
  }
  c->rlaunch_up.swap(c->rlaunch);  // keeps the host table alive for the async copy
  c->rlaunch.clear();
  const size_t tb = c->rlaunch_up.size() * sizeof(RerunLaunch);
  HIP_TRY(c->rtab.ensure(tb));
  HIP_TRY(hipMemcpyAsync(c->rtab.p, c->rlaunch_up.data(), tb, hipMemcpyHostToDevice, c->stream));
  uint32_t* qn = (uint32_t*)((char*)c->rq.p + (size_t)kRerunQueue * 8);
  // how many episodes the launches queued (a flush is a synchronization point anyway). Up to
  // one per CU: one-wave workgroups of 512 with the lane's heap, visibility and scratch in up
  // to a whole CU's LDS, the fastest per episode (a re-run is one dependent chain). More
  // (the headline's sweep queues ~140 per step, ~2,850 in a 20-step timed region, half of
  // them gamma = 0 re-runs whose +inf messages keep the heap large): LDS of that size would
  // run them one CU at a time, round after round, so each episode gets a workgroup of its own
  // with its region in HBM instead and they all run at once
  int64_t lanes = kRerunLanes, lds_rest = rest;
#ifndef CPR_FLUSH_ADAPTIVE
#define CPR_FLUSH_ADAPTIVE 1
#endif
  if (CPR_FLUSH_ADAPTIVE) {
    HIP_TRY(hipStreamSynchronize(c->stream));
    uint32_t nq = 0;
    HIP_TRY(hipMemcpy(&nq, qn, sizeof(nq), hipMemcpyDeviceToHost));
    if ((int64_t)nq > (int64_t)c->cus) {
      lanes = std::min<int64_t>((int64_t)nq, kRerunLanesMax);
      lds_rest = 0;
      // A/B: LDS per workgroup in this mode (the heap at the capacity that fits, an episode
      // that outgrows it again in HBM); 0 = the whole region in HBM
      if (const char* v = getenv("CPR_RERUN_WIDE_LDS")) lds_rest = std::min<int64_t>(rest, atoll(v));
    }
  }
  if (c->rmem.ensure((size_t)lanes * (size_t)lb) != hipSuccess) {
    // the wide grid's regions do not fit: the default grid (its LDS mode), episodes looping
    // over its workgroups, rather than failing the caller's synchronization
    (void)hipGetLastError();
    lanes = kRerunLanes;
    lds_rest = rest;
    HIP_TRY(c->rmem.ensure((size_t)lanes * (size_t)lb));
  }
  if (const int rc = drain_flush_recs(c, false)) return rc;
  cpr_ctx::FlushRec fr;
  if (!c->fl_free.empty()) {
    fr = c->fl_free.back();
    c->fl_free.pop_back();
  } else {
    HIP_TRY(hipEventCreate(&fr.e0));
    HIP_TRY(hipEventCreate(&fr.e1));
    HIP_TRY(hipEventCreate(&fr.e2));
    HIP_TRY(hipHostMalloc((void**)&fr.cnt, sizeof(uint32_t)));
  }
  HIP_TRY(hipEventRecord(fr.e0, c->stream));
  HIP_TRY(launch_nak_exact_rerun((const RerunLaunch*)c->rtab.p, (int64_t)c->rlaunch_up.size(),
                                 (const int64_t*)c->rq.p, qn, c->rq_cap, (uint8_t*)c->rmem.p,
                                 lb, lds_rest, lanes, c->stream));
  HIP_TRY(hipEventRecord(fr.e1, c->stream));
  HIP_TRY(hipMemcpyAsync(fr.cnt, qn, sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(hipEventRecord(fr.e2, c->stream));
  c->fl_pending.push_back(fr);
  HIP_TRY(hipMemsetAsync(qn, 0, 4, c->stream));
  c->ovf_chunk = 0;  // the next launches' flags follow these re-runs on the stream
  c->ovf_used = 0;
  return CPR_OK;
}

// Whether `count` launches of n_eps episodes can register (register_rerun) one after the
// other without any of them forcing a flush: room in the launch table, the queue capacity as
// it stands, and overflow flags for all of them in the chunks that are there or may still be
// added. (The same walk over the chunks as register_rerun's.)
static bool rerun_room(const cpr_ctx* c, int64_t n_eps, int count) {
  int64_t cap = kRerunQueue;
  if (const char* v = getenv("CPR_RERUN_QUEUE_CAP"))
    cap = std::max<int64_t>(0, std::min<int64_t>(kRerunQueue, atoll(v)));
  if (cap != c->rq_cap && !c->rlaunch.empty()) return false;
  if (c->rlaunch.size() + (size_t)count > kRerunMaxLaunches) return false;
  const size_t need = align256((size_t)std::max<int64_t>(1, n_eps));
  const size_t fresh = std::max(need, (size_t)256 << 20);  // a chunk added for this need
  size_t chunk = c->ovf_chunk, used = c->ovf_used, chunks = c->ovf.size();
  for (int i = 0; i < count; ++i) {
    while (chunk < chunks &&
           used + need > (chunk < c->ovf.size() ? c->ovf[chunk]->bytes : fresh)) {
      ++chunk;
      used = 0;
    }
    if (chunk == chunks) {
      if (chunks >= kOvfMaxChunks) return false;
      ++chunks;
    }
    used += need;
  }
  return true;
}

// A launch whose flagged episodes the exact event engine re-runs at the next
// synchronization point (flush_reruns): its parameters (EP: the Ethereum lane, in Nakamoto
// mode for the closed-form Nakamoto lane), stream and outputs join the context's table;
// the kernel appends (launch_id << 40) | (episode << 8) | flags to the queue
static int register_rerun(cpr_batch* b, const eth::EthParams& EP, int64_t lane_bytes,
                          uint64_t first, const TraceSource* tr, cpr_episode_record* rec_dev,
                          cpr_summary* sum_dev, int64_t n_eps, int64_t** redo,
                          uint32_t** redo_n, uint32_t* launch_id, uint8_t** ovf,
                          const NakParams* hybrid = nullptr) {
  cpr_ctx* c = b->ctx;
  const size_t need = align256((size_t)std::max<int64_t>(1, n_eps));
  // tests force a small queue (CPR_RERUN_QUEUE_CAP) to exercise the overflow flags; a new
  // capacity takes effect at a flush (all launches of one flush share it)
  int64_t cap = kRerunQueue;
  if (const char* v = getenv("CPR_RERUN_QUEUE_CAP"))
    cap = std::max<int64_t>(0, std::min<int64_t>(kRerunQueue, atoll(v)));
  if (cap != c->rq_cap) {
    int rc = flush_reruns(c);
    if (rc) return rc;
    c->rq_cap = cap;
  }
  if (c->rlaunch.size() >= kRerunMaxLaunches) {
    int rc = flush_reruns(c);
    if (rc) return rc;
  }
  // the launch's flags: the rest of the current chunk, else the next chunk that holds them
  // (a new one if none does; earlier chunks stay, queued kernels may still read them).
  // Chunks are reused from the first after every flush; once kOvfMaxChunks are taken the
  // launches so far are flushed first, so many large asynchronous launches between two
  // synchronizations do not keep adding chunks for the life of the context
  for (int pass = 0;; ++pass) {
    while (c->ovf_chunk < c->ovf.size() && c->ovf_used + need > c->ovf[c->ovf_chunk]->bytes) {
      ++c->ovf_chunk;
      c->ovf_used = 0;
    }
    if (c->ovf_chunk < c->ovf.size() || c->ovf.size() < kOvfMaxChunks || pass > 0) break;
    const int rc = flush_reruns(c);  // resets ovf_chunk / ovf_used to chunk 0
    if (rc) return rc;
  }
  if (c->ovf_chunk == c->ovf.size()) {
    c->ovf.emplace_back(new DevBuf());
    HIP_TRY(c->ovf.back()->ensure(std::max(need, (size_t)256 << 20)));
  }
  *ovf = (uint8_t*)c->ovf[c->ovf_chunk]->p + c->ovf_used;
  HIP_TRY(hipMemsetAsync(*ovf, 0, need, c->stream));
  c->ovf_used += need;
  if (!c->rq.p) {
    HIP_TRY(c->rq.ensure((size_t)kRerunQueue * 8 + 64));
    // launch counter and the cumulative HBM-retry counter (cpr_rerun_hbm_retries)
    HIP_TRY(hipMemsetAsync((char*)c->rq.p + (size_t)kRerunQueue * 8, 0, 8, c->stream));
  }
  RerunLaunch rl;
  memset(&rl, 0, sizeof(rl));
  rl.P = EP;
  rl.P.next = nullptr;
  rl.seed = b->cfg.seed;
  rl.first = first;
  rl.is_trace = tr ? 1 : 0;
  if (tr) rl.tr = *tr;
  rl.recs = rec_dev;
  rl.sum = sum_dev;
  rl.lane_bytes = lane_bytes;
  rl.ovf = *ovf;
  rl.n_eps = n_eps;
  if (hybrid) {  // nak_hybrid.h: the closed form's state after the engine's region
    rl.NP = *hybrid;
    rl.hybrid = 1;
    rl.lane_bytes = lane_bytes + hybrid_bytes(hybrid->cap);
  }
  *launch_id = (uint32_t)c->rlaunch.size();
  c->rlaunch.push_back(rl);
  *redo = (int64_t*)c->rq.p;
  *redo_n = (uint32_t*)((char*)c->rq.p + (size_t)kRerunQueue * 8);
  return CPR_OK;
}

// The window lane (eth_window.h) takes Ethereum gym episodes on the selfish-mining network
// whose whole episode fits its block ring: the ring does not wrap (WinLane::append fails
// instead), so an episode of max_steps + 1 activations (+ genesis) must fit cap_b, or every
// episode would end in W_REDO and a one-lane exact re-run. max_progress / max_time only end
// episodes earlier (each lane leaves its loop on its own done). CPR_ETH_WINDOW=0 sends them
// to the event engine instead (A/B runs)
static bool eth_window_ok(const cpr_batch* b) {
  const char* v = getenv("CPR_ETH_WINDOW");
  return (v == nullptr || atoi(v) != 0) && ethw::win_supported(b->EP) &&
         b->EP.max_steps <= (int64_t)b->EP.cap_b - 2;
}

static int run_async_ethwin(cpr_batch* b, int64_t n, uint64_t first, cpr_summary* sum_dev,
                            cpr_episode_record* rec_dev) {
  const int64_t wbytes = ethw::win_lane_bytes(b->EP.cap_b);
  const int64_t full = (int64_t)b->ctx->cus * eth_win_blocks_per_cu(rec_dev != nullptr) * 256;
  const int64_t budget = kLaneBudget / wbytes;
  int64_t lanes = std::min(full, std::max<int64_t>(256, budget));
  lanes = std::max<int64_t>(256, (lanes / 256) * 256);
  // equal rounds of the resident grid (every episode has the same trip count)
  const int64_t rounds = std::max<int64_t>(1, (n + lanes - 1) / lanes);
  lanes = std::max<int64_t>(256, std::min(lanes, ((n + rounds - 1) / rounds + 255) / 256 * 256));
  b->last_lanes = lanes;
  b->last_resident = full;
  void* mem = nullptr;
  HIP_TRY(ctx_pool(b->ctx, (size_t)lanes * (size_t)wbytes, &mem));
  if (!b->ev0) {
    HIP_TRY(hipEventCreate(&b->ev0));
    HIP_TRY(hipEventCreate(&b->ev1));
  }
  int64_t* redo = nullptr;
  uint32_t* redo_n = nullptr;
  uint32_t launch_id = 0;
  uint8_t* ovf = nullptr;
  const int rc = register_rerun(b, b->EP, b->eth_bytes, first, nullptr, rec_dev, sum_dev, n,
                                &redo, &redo_n, &launch_id, &ovf);
  if (rc) return rc;
  // episodes beyond the first round from the context's work queue (a lane that finishes
  // early takes the next); CPR_NAK_WQ=0 keeps the static grid stride (A/B)
  eth::EthParams EP = b->EP;
  const char* wq = getenv("CPR_NAK_WQ");
  if (!(wq && wq[0] == '0')) HIP_TRY(ctx_next(b->ctx, &EP.next));
  HIP_TRY(hipEventRecord(b->ev0, b->ctx->stream));
  HIP_TRY(launch_eth_win_episodes(EP, b->cfg.seed, first, n, (uint8_t*)mem, wbytes, lanes,
                                  rec_dev, sum_dev, redo, redo_n, launch_id, b->ctx->rq_cap,
                                  ovf, b->ctx->stream));
  HIP_TRY(hipEventRecord(b->ev1, b->ctx->stream));
  return CPR_OK;
}

// Ethereum lanes: resident capacity bounded by kLaneBudget for the per-lane regions
static int run_async_eth(cpr_batch* b, int64_t n, uint64_t first, const TraceSource* tr,
                         cpr_summary* sum_dev, cpr_episode_record* rec_dev) {
  if (!tr && !b->nak_ev && eth_window_ok(b)) return run_async_ethwin(b, n, first, sum_dev, rec_dev);
  const int64_t full = (int64_t)b->ctx->cus * eth_blocks_per_cu() * 256;
  const int64_t budget = kLaneBudget / b->eth_bytes;
  int64_t lanes = std::min(full, std::max<int64_t>(256, budget));
  lanes = std::min(lanes, ((n + 255) / 256) * 256);
  lanes = std::max<int64_t>(256, (lanes / 256) * 256);
  b->last_lanes = lanes;
  b->last_resident = full;
  void* mem = nullptr;
  HIP_TRY(ctx_pool(b->ctx, (size_t)lanes * (size_t)b->eth_bytes, &mem));
  if (!b->ev0) {
    HIP_TRY(hipEventCreate(&b->ev0));
    HIP_TRY(hipEventCreate(&b->ev1));
  }
  eth::EthParams EP = b->EP;
  HIP_TRY(ctx_next(b->ctx, &EP.next));
  HIP_TRY(hipEventRecord(b->ev0, b->ctx->stream));
  if (tr)
    HIP_TRY(launch_eth_replay_episodes(EP, *tr, n, (uint8_t*)mem, b->eth_bytes,
                                       lanes, rec_dev, sum_dev, b->ctx->stream));
  else
    HIP_TRY(launch_eth_run_episodes(EP, b->cfg.seed, first, n, (uint8_t*)mem,
                                    b->eth_bytes, lanes, rec_dev, sum_dev, b->ctx->stream));
  HIP_TRY(hipEventRecord(b->ev1, b->ctx->stream));
  return CPR_OK;
}

// B_k / Tailstorm lanes: resident capacity bounded by kLaneBudget for the per-lane regions
static int run_async_bk(cpr_batch* b, int64_t n, uint64_t first, const TraceSource* tr,
                        cpr_summary* sum_dev, cpr_episode_record* rec_dev) {
  const bool tsp = b->cfg.protocol == CPR_PROTO_TAILSTORM;
  const int64_t full = (int64_t)b->ctx->cus * (tsp ? ts_blocks_per_cu() : bk_blocks_per_cu()) * 256;
  const int64_t budget = kLaneBudget / b->bk_bytes;
  int64_t lanes = std::min(full, std::max<int64_t>(256, budget));
  lanes = std::min(lanes, ((n + 255) / 256) * 256);
  lanes = std::max<int64_t>(256, (lanes / 256) * 256);
  b->last_lanes = lanes;
  b->last_resident = full;
  void* pool = nullptr;
  HIP_TRY(ctx_pool(b->ctx, (size_t)lanes * (size_t)b->bk_bytes, &pool));
  if (!b->ev0) {
    HIP_TRY(hipEventCreate(&b->ev0));
    HIP_TRY(hipEventCreate(&b->ev1));
  }
  ts::TsParams TP = b->TP;
  bk::BkParams BP = b->BP;
  HIP_TRY(ctx_next(b->ctx, tsp ? &TP.next : &BP.next));
  HIP_TRY(hipEventRecord(b->ev0, b->ctx->stream));
  uint8_t* mem = (uint8_t*)pool;
  hipStream_t st = b->ctx->stream;
  if (tsp && tr)
    HIP_TRY(launch_ts_replay_episodes(TP, *tr, n, mem, b->bk_bytes, lanes, rec_dev, sum_dev, st));
  else if (tsp)
    HIP_TRY(launch_ts_run_episodes(TP, b->cfg.seed, first, n, mem, b->bk_bytes, lanes, rec_dev,
                                   sum_dev, st));
  else if (tr)
    HIP_TRY(launch_bk_replay_episodes(BP, *tr, n, mem, b->bk_bytes, lanes, rec_dev, sum_dev, st));
  else
    HIP_TRY(launch_bk_run_episodes(BP, b->cfg.seed, first, n, mem, b->bk_bytes, lanes, rec_dev,
                                   sum_dev, st));
  HIP_TRY(hipEventRecord(b->ev1, b->ctx->stream));
  return CPR_OK;
}

// tr == NULL: episodes [first, first + n) of the keyed stream; else trace episodes [0, n)
// FC16 abstract-model episodes: grid-stride over n, a few resident workgroups per CU
static int run_async_fc16(cpr_batch* b, int64_t n, uint64_t first, const TraceSource* tr,
                          cpr_summary* sum_dev, cpr_episode_record* rec_dev) {
  if (tr) return fail(CPR_E_UNSUPPORTED, "FC16 episodes have no trace format");
  int64_t lanes = std::min<int64_t>((int64_t)b->ctx->cus * 8 * 256, ((n + 255) / 256) * 256);
  lanes = std::max<int64_t>(256, lanes);
  if (!b->ev0) {
    HIP_TRY(hipEventCreate(&b->ev0));
    HIP_TRY(hipEventCreate(&b->ev1));
  }
  HIP_TRY(hipEventRecord(b->ev0, b->ctx->stream));
  HIP_TRY(launch_fc16_episodes(b->FP, b->cfg.seed, first, n, lanes, rec_dev, sum_dev,
                               b->ctx->stream));
  HIP_TRY(hipEventRecord(b->ev1, b->ctx->stream));
  return CPR_OK;
}

// whether the exact re-runs of this batch's flagged episodes are hybrid ones (see run_async),
// and the closed form's parameters for them
static bool rerun_hybrid(const cpr_batch* b, bool trace, NakParams* NP) {
  const char* hv = getenv("CPR_RERUN_HYBRID");
  const bool hyb = !(hv && hv[0] == '0') && !trace && b->cfg.mode == CPR_MODE_GYM &&
                   b->cfg.network == CPR_NET_SELFISH_MINING && b->P.arrive == 1 &&
                   !b->P.abstract_g && b->cfg.policy != CPR_POLICY_RANDOM &&
                   !(b->P.max_progress < __builtin_inf()) &&
                   !(b->P.max_time < __builtin_inf()) &&
                   b->NEP.max_steps < (1 << 20) &&
                   b->NEP.max_steps + 2 <= (int64_t)b->NEP.cap_b;
  *NP = b->P;
  NP->cap = (int32_t)((b->NEP.max_steps + 2 + 63) / 64 * 64);
  return hyb;
}

static const char* kGenericNoFused =
    "generic env: no built-in policy runs its episodes (no fused kernel); step the lanes "
    "(cpr_step) or roll out a network (cpr_rollout_net)";

static int run_async(cpr_batch* b, int64_t n, uint64_t first, const TraceSource* tr,
                     cpr_summary* sum_dev, cpr_episode_record* rec_dev) {
  if (b->is_fc16) return run_async_fc16(b, n, first, tr, sum_dev, rec_dev);
  if (b->gen_env) return fail(CPR_E_UNSUPPORTED, kGenericNoFused);
  if (b->cfg.protocol == CPR_PROTO_ETHEREUM || b->nak_ev)
    return run_async_eth(b, n, first, tr, sum_dev, rec_dev);
  if (b->is_ev) return run_async_bk(b, n, first, tr, sum_dev, rec_dev);
  const int bpc = run_episodes_blocks_per_cu(b->P, b->cfg.mode, rec_dev != nullptr);
  const int64_t lanes = episode_lanes(b, n, bpc);
  b->last_lanes = lanes;
  b->last_resident = (int64_t)b->ctx->cus * bpc * 256;
  b->fuse_time.reset();
  // spill [lane][cap] f64 mining times | tie-replay scratch [lane] | the deferred-race
  // kernel's second-pass list (1 + n words)
  const size_t o_replay = align256((size_t)lanes * b->P.cap * sizeof(double));
  const size_t o_list = align256(o_replay + (size_t)lanes * REPLAY_BYTES);
  const size_t list_bytes = tr ? 0 : (size_t)run_episodes_list_bytes(b->P, b->cfg.mode,
                                                                      rec_dev != nullptr, n);
  // the second pass of a deferred-race launch runs on the side stream (cpr_ctx.side) with
  // its list in one of the context's two list buffers; CPR_SIDE_PASS=0 keeps it on the
  // stream with the list in the pool (A/B)
  const char* sp = getenv("CPR_SIDE_PASS");
  const bool side = list_bytes > 0 && !(sp && sp[0] == '0');
  cpr_ctx* c = b->ctx;
  void* pool = nullptr;
  HIP_TRY(ctx_pool(c, side ? o_list : o_list + list_bytes, &pool));
  double* spill = (double*)pool;
  uint8_t* replay = (uint8_t*)pool + o_replay;
  int64_t* list = list_bytes ? (int64_t*)((uint8_t*)pool + o_list) : nullptr;
  const int li = c->list_i;
  if (side) {
    if (c->list_pending[li]) {
      // the pass that reads this buffer (two launches ago) must be done before the main
      // kernel rewrites it; before a reallocation, on the host
      if (c->lists[li].bytes < list_bytes) HIP_TRY(hipEventSynchronize(c->list_ev[li]));
      HIP_TRY(hipStreamWaitEvent(c->stream, c->list_ev[li], 0));
      c->list_pending[li] = false;
    }
    HIP_TRY(c->lists[li].ensure(list_bytes));
    list = (int64_t*)c->lists[li].p;
  }
  if (!b->ev0) {
    HIP_TRY(hipEventCreate(&b->ev0));
    HIP_TRY(hipEventCreate(&b->ev1));
  }
  int64_t* redo = nullptr;
  uint32_t* redo_n = nullptr;
  uint32_t launch_id = 0;
  uint8_t* ovf = nullptr;
  if (b->has_rerun) {
    // hybrid re-runs (nak_hybrid.h) where a quiescent point has the reference's queue state:
    // gym episodes on the selfish-mining network whose attacker messages arrive (gamma > 0),
    // ended by max_steps alone, the whole episode in the engine's block ring, a seeded
    // stream and a deterministic policy; CPR_RERUN_HYBRID=0 re-runs whole episodes (A/B)
    NakParams NP;
    const bool hyb = rerun_hybrid(b, tr != nullptr, &NP);
    const int rc = register_rerun(b, b->NEP, b->nak_bytes, first, tr, rec_dev, sum_dev, n,
                                  &redo, &redo_n, &launch_id, &ovf, hyb ? &NP : nullptr);
    if (rc) return rc;
  }
  HIP_TRY(hipEventRecord(b->ev0, b->ctx->stream));
  if (tr)
    HIP_TRY(launch_replay_episodes(b->P, *tr, n, b->cfg.mode, b->cfg.activations,
                                   spill, replay, lanes, rec_dev, sum_dev, redo, redo_n,
                                   launch_id, b->ctx->rq_cap, ovf, b->ctx->stream));
  else {
    // the fused kernel's work queue (kernels.hip nak_next_episode); CPR_NAK_WQ=0 keeps the
    // static grid stride (A/B)
    NakParams P = b->P;
    const char* wq = getenv("CPR_NAK_WQ");
    if (!(wq && wq[0] == '0')) HIP_TRY(ctx_next(b->ctx, &P.next));
    bool ran = false;
    const SidePass sd{c->side, c->main_ev, c->list_ev[li], &ran};
    HIP_TRY(launch_run_episodes(P, b->cfg.seed, first, n, b->cfg.mode, b->cfg.activations,
                                spill, replay, list, lanes, rec_dev, sum_dev, redo, redo_n,
                                launch_id, b->ctx->rq_cap, ovf, b->ctx->stream,
                                side ? &sd : nullptr));
    if (ran) {
      c->list_pending[li] = true;
      c->list_i ^= 1;
      // the launch's time spans both kernels: ev0 on the stream, ev1 behind the second pass
      HIP_TRY(hipEventRecord(b->ev1, c->side));
      return CPR_OK;
    }
  }
  HIP_TRY(hipEventRecord(b->ev1, b->ctx->stream));
  return CPR_OK;
}

// ---- sweep points that share their draws: one k_run_episodes_fused launch per group

// the largest group (CPR_NAK_FUSE, read at every call; 0 or 1: every call launches at once)
#ifndef CPR_NAK_FUSE_DEFAULT
#define CPR_NAK_FUSE_DEFAULT CPR_NAK_FUSE_MAX
#endif
#ifndef CPR_NAK_FUSE_DEFAULT_ARR  // the deferred-race (gamma = .5) kernel's
#define CPR_NAK_FUSE_DEFAULT_ARR CPR_NAK_FUSE_MAX_ARR
#endif
static int fuse_cap(int kind) {
  int cap = kind == 2 ? CPR_NAK_FUSE_DEFAULT_ARR : CPR_NAK_FUSE_DEFAULT;
  if (const char* v = getenv("CPR_NAK_FUSE")) cap = atoi(v);
  return std::max(0, std::min(cap, kind == 2 ? kFuseMaxArr : kFuseMax));
}

// the lanes of a lane group (nak_fused.h): the largest built power of two that
// CPR_NAK_FUSE_LANES (read at every call) allows; 1: none, every lane its own episode. Lane
// groups are built with full lanes only, so a smaller CPR_NAK_FUSE leaves none
static int fuse_lanes(int kind, int cap) {
  if (cap < 1 || cap != (kind == 2 ? kFuseMaxArr : kFuseMax)) return 1;
  int g = kind == 2 ? kFuseLanesArr : kFuseLanes;
  if (const char* v = getenv("CPR_NAK_FUSE_LANES")) g = std::min(g, atoi(v));
  int p = 1;
  while (2 * p <= g) p *= 2;
  return p;
}

// which of the instantiations the fused kernel stands for a call would run (0: neither)
static int fuse_kind(const cpr_batch* b, const cpr_episode_record* rec_dev) {
  if (b->cfg.protocol != CPR_PROTO_NAKAMOTO || b->nak_ev || b->is_ev || b->is_eth) return 0;
  const int kind = run_episodes_fusable(b->P, b->cfg.mode, rec_dev != nullptr);
  // k_run_episodes_fused makes no capacity test (LaneMem::cap_test): an episode's
  // max_steps + 1 activations must fit below cap. nak_params always sizes cap so; this keeps
  // the premise where it is relied on (a fusable launch has max_steps <= 2^14, lazy_clock_ok)
  if (kind != 0 && (int64_t)b->P.cap < b->P.max_steps + 2) return 0;
  // the deferred-race group's second passes run on the side stream only (CPR_SIDE_PASS=0:
  // every call launches at once, its second pass on the stream)
  const char* sp = getenv("CPR_SIDE_PASS");
  return kind == 2 && sp && sp[0] == '0' ? 0 : kind;
}

// the same launch but for alpha: every field the kernel and the launcher read except t_att,
// the seed, and what the exact re-runs of flagged episodes depend on
static bool fuse_same_launch(const cpr_batch* a, const cpr_batch* b) {
  const NakParams &P = a->P, &Q = b->P;
  return a->ctx == b->ctx && a->cfg.seed == b->cfg.seed && a->cfg.mode == b->cfg.mode &&
         a->cfg.network == b->cfg.network && a->cfg.policy == b->cfg.policy &&
         P.policy == Q.policy && P.d == Q.d && P.arrive == Q.arrive && P.ev == Q.ev &&
         P.delta == Q.delta && P.dmax == Q.dmax && P.max_steps == Q.max_steps &&
         P.max_progress == Q.max_progress && P.max_time == Q.max_time && P.cap == Q.cap &&
         P.abstract_g == Q.abstract_g && a->has_rerun == b->has_rerun &&
         a->nak_bytes == b->nak_bytes && a->NEP.max_steps == b->NEP.max_steps &&
         a->NEP.cap_b == b->NEP.cap_b && a->NEP.cap_e == b->NEP.cap_e && a->NEP.n == b->NEP.n;
}

// one k_run_episodes_fused launch: na points per lane, gl lanes per episode, np = na * gl
// members (np >= 2)
static int fuse_launch_group(cpr_ctx* c, const cpr_ctx::FuseMember* g, int na, int gl, int kind,
                             int64_t n, uint64_t first) {
  const int np = na * gl;
  cpr_batch* b0 = g[0].b;
  // every member's re-run registration before the kernel. A flush in the middle would drop
  // the registrations made so far, so where the launch table or the overflow-flag chunks
  // may not hold the whole group, the flush comes first, before the group's kernel on the
  // stream, and the group registers into the emptied table
  FusePoint pts[kFusePoints];
  int64_t* redo = nullptr;
  uint32_t* redo_n = nullptr;
  if (b0->has_rerun) {
    if (!rerun_room(c, n, np)) {
      if (const int rc = flush_reruns(c)) return rc;
    }
    for (int i = 0; i < np; ++i) {
      cpr_batch* b = g[i].b;
      NakParams NP;
      const bool hyb = rerun_hybrid(b, false, &NP);
      if (const int rc = register_rerun(b, b->NEP, b->nak_bytes, first, nullptr, nullptr,
                                        g[i].sum, n, &redo, &redo_n, &pts[i].launch_id,
                                        &pts[i].ovf, hyb ? &NP : nullptr))
        return rc;
    }
    if (pts[np - 1].launch_id != pts[0].launch_id + (uint32_t)(np - 1))
      return fail(CPR_E_HIP, "re-run table flushed while a group registered");
  }
  // deferred races: one list region per member in one of the context's two list buffers
  // (run_async), read by the members' eager second passes on the side stream
  const size_t list_bytes =
      kind == 2 ? align256((size_t)run_episodes_list_bytes(b0->P, b0->cfg.mode, false, n)) : 0;
  const int li = c->list_i;
  if (kind == 2) {
    if (c->list_pending[li]) {
      if (c->lists[li].bytes < list_bytes * np) HIP_TRY(hipEventSynchronize(c->list_ev[li]));
      HIP_TRY(hipStreamWaitEvent(c->stream, c->list_ev[li], 0));
      c->list_pending[li] = false;
    }
    HIP_TRY(c->lists[li].ensure(list_bytes * np));
  }
  for (int i = 0; i < np; ++i) {
    pts[i].t_att = g[i].b->P.t_att;
    pts[i].sum = g[i].sum;
    pts[i].list = kind == 2 ? (int64_t*)((uint8_t*)c->lists[li].p + list_bytes * i) : nullptr;
    if (!b0->has_rerun) {
      pts[i].ovf = nullptr;
      pts[i].launch_id = 0;
    }
  }
  const int bpc = run_episodes_fused_blocks_per_cu(b0->P, na, gl);
  // gl lanes per episode
  const int64_t lanes = episode_lanes(b0, n * gl, bpc);
  auto ft = std::make_shared<FuseTime>();
  ft->size = np;
  HIP_TRY(hipEventCreate(&ft->ev0));
  HIP_TRY(hipEventCreate(&ft->ev1));
  NakParams P = b0->P;
  const char* wq = getenv("CPR_NAK_WQ");
  if (!(wq && wq[0] == '0')) HIP_TRY(ctx_next(c, &P.next));
  HIP_TRY(hipEventRecord(ft->ev0, c->stream));
  HIP_TRY(launch_run_episodes_fused(P, b0->cfg.seed, first, n, pts, na, gl, lanes, redo, redo_n,
                                    c->rq_cap, c->stream));
  // the group's time is its kernel's, on the stream. The second passes below are not in it:
  // on the side stream they share the device with the next launch and mostly wait for its
  // workgroups to leave, so a span that ended behind them would hold that launch as well
  HIP_TRY(hipEventRecord(ft->ev1, c->stream));
  if (kind == 2) {
    // every member's eager second pass, an unfused launch with the member's own alpha, on
    // the side stream behind the group's kernel: they overlap the next launch on the stream
    const int64_t lanes2 =
        episode_lanes(b0, n, run_episodes_blocks_per_cu(b0->P, b0->cfg.mode, false));
    HIP_TRY(hipEventRecord(c->main_ev, c->stream));
    HIP_TRY(hipStreamWaitEvent(c->side, c->main_ev, 0));
    for (int i = 0; i < np; ++i)
      HIP_TRY(launch_run_episodes_second(g[i].b->P, b0->cfg.seed, first, n, pts[i].list, lanes2,
                                         g[i].sum, redo, redo_n, pts[i].launch_id, c->rq_cap,
                                         pts[i].ovf, c->side));
    HIP_TRY(hipEventRecord(c->list_ev[li], c->side));
    c->list_pending[li] = true;
    c->list_i ^= 1;
  }
  for (int i = 0; i < np; ++i) {
    cpr_batch* b = g[i].b;
    b->last_lanes = lanes;
    b->last_resident = (int64_t)c->cus * bpc * 256;
    b->fuse_time = ft;
    b->async_launch = true;
  }
  return CPR_OK;
}

// The pending members, in call order, cut greedily: first into full lane-group launches
// (every lane full: NAmax points per lane x the largest lane group CPR_NAK_FUSE_LANES
// allows), the rest into groups of up to NAmax points in one lane each, a single member as
// the one-point kernel
static int fuse_launch_pending(cpr_ctx* c) {
  if (c->fuse.empty()) return CPR_OK;
  // emptied first: whatever fails below, the group is not launched twice
  std::vector<cpr_ctx::FuseMember> g;
  g.swap(c->fuse);
  const int64_t n = c->fuse_n;
  const uint64_t first = c->fuse_first;
  HIP_TRY(hipSetDevice(c->device));
  const int kind = c->fuse_kind;
  const int namax = std::max(1, fuse_cap(kind));
  int gl = fuse_lanes(kind, namax);
  const int m = (int)g.size();
  int i = 0;
  while (i < m) {
    if (m - i < namax * gl) gl = 1;
    const int np = gl > 1 ? namax * gl : std::min(namax, m - i);
    if (np == 1) {
      g[i].b->async_launch = true;
      if (const int rc = run_async(g[i].b, n, first, nullptr, g[i].sum, nullptr)) return rc;
    } else if (const int rc = fuse_launch_group(c, &g[i], gl > 1 ? namax : np, gl, kind, n,
                                                first)) {
      return rc;
    }
    i += np;
  }
  return CPR_OK;
}

int cpr_run_episodes_async(cpr_batch* b, int64_t n, uint64_t first, cpr_summary* sum_dev,
                           cpr_episode_record* rec_dev) {
  if (!b || !sum_dev) return fail(CPR_E_INVALID_ARG, "NULL argument");
  if (b->gen_env) return fail(CPR_E_UNSUPPORTED, kGenericNoFused);
  if (n <= 0) return CPR_OK;
  cpr_ctx* c = b->ctx;
  const int kind = fuse_kind(b, rec_dev);
  const int cap = fuse_cap(kind);
  // (a build with one point per lane groups through its lane groups alone)
  const bool fusable = kind != 0 && cap >= 1 && cap * fuse_lanes(kind, cap) >= 2;
  // the pending group is launched before any call that does not join it is handled
  if (!c->fuse.empty() && !(fusable && n == c->fuse_n && first == c->fuse_first &&
                            fuse_same_launch(c->fuse[0].b, b)))
    CPR_ENTER(c);
  if (fusable) {
    c->fuse.push_back({b, sum_dev});
    c->fuse_kind = kind;
    c->fuse_n = n;
    c->fuse_first = first;
    // the pending group grows to one full lane-group launch (points per lane x lanes)
    if ((int)c->fuse.size() >= cap * fuse_lanes(kind, cap)) CPR_ENTER(c);
    return CPR_OK;
  }
  HIP_TRY(hipSetDevice(c->device));
  b->async_launch = true;
  return run_async(b, n, first, nullptr, sum_dev, rec_dev);
}

static int run_sync(cpr_batch* b, int64_t n, uint64_t first, const TraceSource* tr,
                    cpr_summary* summary, cpr_episode_record* records, int records_on_device) {
  hipStream_t st = b->ctx->stream;
  HIP_TRY(b->summary.ensure(sizeof(cpr_summary)));
  HIP_TRY(hipMemsetAsync(b->summary.p, 0, sizeof(cpr_summary), st));
  cpr_episode_record* rec_dev = nullptr;
  if (records) {
    if (records_on_device)
      rec_dev = records;
    else {
      HIP_TRY(b->records.ensure((size_t)n * sizeof(cpr_episode_record)));
      rec_dev = (cpr_episode_record*)b->records.p;
    }
  }
  int rc = run_async(b, n, first, tr, (cpr_summary*)b->summary.p, rec_dev);
  if (rc) return rc;
  rc = flush_reruns(b->ctx);
  if (rc) return rc;
  cpr_summary s;
  HIP_TRY(hipMemcpyAsync(&s, b->summary.p, sizeof(s), hipMemcpyDeviceToHost, st));
  if (records && !records_on_device)
    HIP_TRY(hipMemcpyAsync(records, rec_dev, (size_t)n * sizeof(cpr_episode_record),
                           hipMemcpyDeviceToHost, st));
  HIP_TRY(hipStreamSynchronize(st));
  float ms = 0.f;
  HIP_TRY(hipEventElapsedTime(&ms, b->ev0, b->ev1));
  b->last_ms = ms;
  b->last_acts = s.activations;
  summary->episodes += s.episodes;
  summary->steps += s.steps;
  summary->activations += s.activations;
  summary->reward_attacker_fx += s.reward_attacker_fx;
  summary->reward_defender_fx += s.reward_defender_fx;
  summary->progress_fx += s.progress_fx;
  summary->rel_revenue_fx += s.rel_revenue_fx;
  summary->rel_revenue_sq_fx += s.rel_revenue_sq_fx;
  summary->orphans += s.orphans;
  summary->status_tie += s.status_tie;
  summary->status_overlap += s.status_overlap;
  summary->status_other += s.status_other;
  summary->invalid += s.invalid;
  for (int i = 0; i < CPR_HIST_BINS; i++) summary->hist[i] += s.hist[i];
  return CPR_OK;
}

int cpr_run_episodes(cpr_batch* b, int64_t n, uint64_t first, cpr_summary* summary,
                     cpr_episode_record* records, int records_on_device) {
  if (!b || !summary) return fail(CPR_E_INVALID_ARG, "NULL argument");
  CPR_ENTER(b->ctx);
  if (b->gen_env) return fail(CPR_E_UNSUPPORTED, kGenericNoFused);
  if (n <= 0) return CPR_OK;
  HIP_TRY(hipSetDevice(b->ctx->device));
  return run_sync(b, n, first, nullptr, summary, records, records_on_device);
}

// host-side checks of a trace before any of it reaches a lane: CSR offsets, miners within
// the network, delays non-negative (not NaN), keys strictly ascending per episode
static int check_trace(const cpr_batch* b, const cpr_trace* t) {
  const int64_t E = t->n_episodes;
  // two agents: 2 nodes; honest clique: exactly `defenders` nodes; selfish mining: the
  // attacker plus `defenders`
  const int32_t nodes = b->cfg.network == CPR_NET_TWO_AGENTS      ? 2
                        : b->cfg.network == CPR_NET_HONEST_CLIQUE ? b->cfg.defenders
                                                                  : b->cfg.defenders + 1;
  const int64_t* offs[3] = {t->act_offset, t->pow_offset, t->link_offset};
  const char* names[3] = {"act_offset", "pow_offset", "link_offset"};
  for (int a = 0; a < 3; a++) {
    const int64_t* o = offs[a];
    const std::string nm = std::string("cpr_trace.") + names[a];
    if (!o) return fail(CPR_E_INVALID_ARG, nm + " is NULL");
    if (o[0] != 0) return fail(CPR_E_INVALID_ARG, nm + "[0] != 0");
    for (int64_t e = 0; e < E; e++)
      if (o[e + 1] < o[e] || o[e + 1] - o[e] > INT32_MAX)
        return fail(CPR_E_INVALID_ARG, nm + " not monotone");
  }
  const int64_t na = t->act_offset[E], np = t->pow_offset[E], nl = t->link_offset[E];
  if ((na && (!t->act_miner || !t->act_delay)) || (np && !t->pow_hash) ||
      (nl && (!t->link_key || !t->link_delay)))
    return fail(CPR_E_INVALID_ARG, "cpr_trace: NULL array with nonzero length");
  for (int64_t i = 0; i < na; i++) {
    if (t->act_miner[i] < 0 || t->act_miner[i] >= nodes)
      return fail(CPR_E_INVALID_ARG, "cpr_trace.act_miner: node index out of range");
    if (!(t->act_delay[i] >= 0.0))
      return fail(CPR_E_INVALID_ARG, "cpr_trace.act_delay: negative or NaN delay");
  }
  for (int64_t i = 0; i < nl; i++)
    if (!(t->link_delay[i] >= 0.0))
      return fail(CPR_E_INVALID_ARG, "cpr_trace.link_delay: negative or NaN delay");
  for (int64_t e = 0; e < E; e++)
    for (int64_t i = t->link_offset[e] + 1; i < t->link_offset[e + 1]; i++)
      if (t->link_key[i] <= t->link_key[i - 1])
        return fail(CPR_E_INVALID_ARG, "cpr_trace.link_key: not strictly ascending");
  return CPR_OK;
}

// copy a checked trace into the batch's trace buffers (on the context's stream)
static int upload_trace(cpr_batch* b, const cpr_trace* t, TraceSource* out) {
  hipStream_t st = b->ctx->stream;
  const int64_t E = t->n_episodes;
  const int64_t na = t->act_offset[E], np = t->pow_offset[E], nl = t->link_offset[E];
  const size_t ob = (size_t)(E + 1) * sizeof(int64_t);
  // one device buffer holds the three offset arrays; empty arrays get 8 bytes
  HIP_TRY(b->tr_off.ensure(3 * ob));
  HIP_TRY(b->tr_miner.ensure(std::max<size_t>(8, (size_t)na * sizeof(int32_t))));
  HIP_TRY(b->tr_delay.ensure(std::max<size_t>(8, (size_t)na * sizeof(double))));
  HIP_TRY(b->tr_pow.ensure(std::max<size_t>(8, (size_t)np * sizeof(int32_t))));
  HIP_TRY(b->tr_key.ensure(std::max<size_t>(8, (size_t)nl * sizeof(uint64_t))));
  HIP_TRY(b->tr_ldelay.ensure(std::max<size_t>(8, (size_t)nl * sizeof(double))));
  char* off = (char*)b->tr_off.p;
  HIP_TRY(hipMemcpyAsync(off, t->act_offset, ob, hipMemcpyHostToDevice, st));
  HIP_TRY(hipMemcpyAsync(off + ob, t->pow_offset, ob, hipMemcpyHostToDevice, st));
  HIP_TRY(hipMemcpyAsync(off + 2 * ob, t->link_offset, ob, hipMemcpyHostToDevice, st));
  if (na) {
    HIP_TRY(hipMemcpyAsync(b->tr_miner.p, t->act_miner, na * sizeof(int32_t),
                           hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(b->tr_delay.p, t->act_delay, na * sizeof(double),
                           hipMemcpyHostToDevice, st));
  }
  if (np)
    HIP_TRY(hipMemcpyAsync(b->tr_pow.p, t->pow_hash, np * sizeof(int32_t), hipMemcpyHostToDevice,
                           st));
  if (nl) {
    HIP_TRY(hipMemcpyAsync(b->tr_key.p, t->link_key, nl * sizeof(uint64_t),
                           hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(b->tr_ldelay.p, t->link_delay, nl * sizeof(double),
                           hipMemcpyHostToDevice, st));
  }
  TraceSource src;
  src.act_off = (const int64_t*)off;
  src.pow_off = (const int64_t*)(off + ob);
  src.link_off = (const int64_t*)(off + 2 * ob);
  src.act_miner = (const int32_t*)b->tr_miner.p;
  src.act_delay = (const double*)b->tr_delay.p;
  src.pow_hash = (const int32_t*)b->tr_pow.p;
  src.link_key = (const uint64_t*)b->tr_key.p;
  src.link_delay = (const double*)b->tr_ldelay.p;
  *out = src;
  return CPR_OK;
}

int cpr_replay(cpr_batch* b, const cpr_trace* t, cpr_summary* summary,
               cpr_episode_record* records, int records_on_device) {
  if (!b || !t || !summary) return fail(CPR_E_INVALID_ARG, "NULL argument");
  CPR_ENTER(b->ctx);
  if (b->fc16_env) return fail(CPR_E_UNSUPPORTED, "FC16 episodes have no trace format");
  if (b->gen_env) return fail(CPR_E_UNSUPPORTED, "generic env episodes have no trace format");
  if (b->cfg.network == CPR_NET_ABSTRACT_GAMMA)
    return fail(CPR_E_UNSUPPORTED, "the abstract-gamma mode has no trace replay");
  if (t->n_episodes <= 0) return CPR_OK;
  int rc = check_trace(b, t);
  if (rc) return rc;
  HIP_TRY(hipSetDevice(b->ctx->device));
  TraceSource src;
  rc = upload_trace(b, t, &src);
  if (rc) return rc;
  return run_sync(b, t->n_episodes, 0, &src, summary, records, records_on_device);
}

static int32_t network_nodes(const cpr_config& c) {
  return c.network == CPR_NET_TWO_AGENTS      ? 2
         : c.network == CPR_NET_HONEST_CLIQUE ? c.defenders
                                               : c.defenders + 1;  // attacker + defenders
}

// Per-node outputs (csv_runner.ml:74-79): the episodes run once more on the exact event
// engine with a second per-lane region holding activations per node and per-block reward
// arrays; Nakamoto configurations of the closed-form lane use the Nakamoto-mode engine of
// the exact re-runs (same episodes, bit for bit)
int cpr_node_outputs(cpr_batch* b, int64_t n, uint64_t first, const cpr_trace* trace,
                     int32_t n_nodes, cpr_episode_record* records, int64_t* node_activations,
                     double* node_rewards) {
  if (!b || !node_activations || !node_rewards) return fail(CPR_E_INVALID_ARG, "NULL argument");
  CPR_ENTER(b->ctx);
  if (b->is_fc16) return fail(CPR_E_UNSUPPORTED, "FC16 episodes have no network nodes");
  if (b->gen_env)
    return fail(CPR_E_UNSUPPORTED, "generic env episodes have two parties, no network nodes");
  if (b->cfg.network == CPR_NET_ABSTRACT_GAMMA)
    return fail(CPR_E_UNSUPPORTED, "the abstract-gamma mode has no exact event engine");
  if (n_nodes != network_nodes(b->cfg))
    return fail(CPR_E_INVALID_ARG, "n_nodes must equal the network's node count");
  const bool nak_fused = b->cfg.protocol == CPR_PROTO_NAKAMOTO && !b->nak_ev;
  if (nak_fused && !b->has_rerun)
    return fail(CPR_E_UNSUPPORTED, "configuration beyond the exact event engine's capacity");
  int rc;
  TraceSource src;
  if (trace) {
    rc = check_trace(b, trace);
    if (rc) return rc;
    n = trace->n_episodes;
    first = 0;
  }
  if (n <= 0) return CPR_OK;
  HIP_TRY(hipSetDevice(b->ctx->device));
  if (trace) {
    rc = upload_trace(b, trace, &src);
    if (rc) return rc;
  }
  hipStream_t st = b->ctx->stream;
  const bool eth = b->cfg.protocol == CPR_PROTO_ETHEREUM || b->cfg.protocol == CPR_PROTO_NAKAMOTO;
  const bool tsp = b->cfg.protocol == CPR_PROTO_TAILSTORM;
  eth::EthParams EP = nak_fused ? b->NEP : b->EP;
  ts::TsParams TP = b->TP;
  bk::BkParams BP = b->BP;
  const int64_t lane_bytes = eth ? eth::eth_lane_bytes(EP.cap_b, EP.cap_e, EP.n) : b->bk_bytes;
  const int64_t node_bytes = eth ? eth::eth_node_bytes(EP.cap_b, EP.n)
                             : tsp ? ts::ts_align((int64_t)b->TP.n * 8)
                                   : bk::bk_node_bytes(b->BP);
  const int64_t per_cu = eth ? eth_blocks_per_cu() : (tsp ? ts_blocks_per_cu() : bk_blocks_per_cu());
  const int64_t full = (int64_t)b->ctx->cus * per_cu * 256;
  const int64_t budget = kLaneBudget / (lane_bytes + node_bytes);
  int64_t lanes = std::min(full, std::max<int64_t>(256, budget));
  lanes = std::min(lanes, ((n + 255) / 256) * 256);
  lanes = std::max<int64_t>(256, (lanes / 256) * 256);
  void* pool = nullptr;
  const size_t o_node = align256((size_t)lanes * (size_t)lane_bytes);
  HIP_TRY(ctx_pool(b->ctx, o_node + (size_t)lanes * (size_t)node_bytes, &pool));
  DevBuf out, sum;
  const size_t rows = (size_t)n * (size_t)n_nodes;
  const size_t o_rew = align256(rows * 8), o_hm = o_rew + align256(rows * 8),
               o_rec = o_hm + align256((size_t)n * 4);
  HIP_TRY(out.ensure(o_rec + (size_t)n * sizeof(cpr_episode_record)));
  HIP_TRY(sum.ensure(sizeof(cpr_summary)));
  HIP_TRY(hipMemsetAsync(sum.p, 0, sizeof(cpr_summary), st));
  NodeOut no;
  no.mem = (uint8_t*)pool + o_node;
  no.lane_bytes = node_bytes;
  no.acts = (int64_t*)out.p;
  no.rews = (double*)((char*)out.p + o_rew);
  no.head_miner = (int32_t*)((char*)out.p + o_hm);
  cpr_episode_record* rec = (cpr_episode_record*)((char*)out.p + o_rec);
  cpr_summary* sd = (cpr_summary*)sum.p;
  uint8_t* mem = (uint8_t*)pool;
  HIP_TRY(ctx_next(b->ctx, eth ? &EP.next : tsp ? &TP.next : &BP.next));
  if (eth && trace)
    HIP_TRY(launch_eth_replay_episodes(EP, src, n, mem, lane_bytes, lanes, rec, sd, st, no));
  else if (eth)
    HIP_TRY(launch_eth_run_episodes(EP, b->cfg.seed, first, n, mem, lane_bytes, lanes, rec, sd,
                                    st, no));
  else if (tsp && trace)
    HIP_TRY(launch_ts_replay_episodes(TP, src, n, mem, lane_bytes, lanes, rec, sd, st, no));
  else if (tsp)
    HIP_TRY(launch_ts_run_episodes(TP, b->cfg.seed, first, n, mem, lane_bytes, lanes, rec, sd,
                                   st, no));
  else if (trace)
    HIP_TRY(launch_bk_replay_episodes(BP, src, n, mem, lane_bytes, lanes, rec, sd, st, no));
  else
    HIP_TRY(launch_bk_run_episodes(BP, b->cfg.seed, first, n, mem, lane_bytes, lanes, rec, sd,
                                   st, no));
  std::vector<int32_t> hm((size_t)n);
  HIP_TRY(hipMemcpyAsync(node_activations, no.acts, rows * 8, hipMemcpyDeviceToHost, st));
  HIP_TRY(hipMemcpyAsync(node_rewards, no.rews, rows * 8, hipMemcpyDeviceToHost, st));
  HIP_TRY(hipMemcpyAsync(hm.data(), no.head_miner, (size_t)n * 4, hipMemcpyDeviceToHost, st));
  if (records)
    HIP_TRY(hipMemcpyAsync(records, rec, (size_t)n * sizeof(cpr_episode_record),
                           hipMemcpyDeviceToHost, st));
  HIP_TRY(hipStreamSynchronize(st));
  if (records)
    for (int64_t e = 0; e < n; e++) records[e].head_miner = hm[(size_t)e];
  return CPR_OK;
}

// ---------------------------------------------------------------- lockstep API

static int obs_len_of(const cpr_config& c) {
  switch (c.protocol) {
    case CPR_PROTO_BK: return 8;
    case CPR_PROTO_ETHEREUM: return 10;
    case CPR_PROTO_TAILSTORM: return 10;
    case CPR_PROTO_FC16_ENV: return 3;
    case CPR_PROTO_GENERIC_NAKAMOTO: return 5;
    default: return 4;
  }
}

static int ensure_common_lockstep(cpr_batch* b, int obs_len) {
  const int64_t n = b->cfg.n_lanes;
  HIP_TRY(b->l_obs.ensure((size_t)n * obs_len * sizeof(double)));
  HIP_TRY(b->l_act.ensure((size_t)n * sizeof(int32_t)));
  HIP_TRY(b->l_rew.ensure((size_t)n * sizeof(double)));
  HIP_TRY(b->l_done.ensure((size_t)n));
  HIP_TRY(b->l_mask.ensure((size_t)n));
  HIP_TRY(b->l_eps.ensure((size_t)n * sizeof(uint64_t)));
  HIP_TRY(b->l_info.ensure((size_t)n * (7 * 8 + 3 * 4)));
  return CPR_OK;
}

// per-lane region bytes of the event-engine lockstep lanes (B_k, Tailstorm, Ethereum)
static int64_t ev_lane_bytes(const cpr_batch* b) { return b->is_eth ? b->eth_bytes : b->bk_bytes; }

static int ensure_lockstep_bk(cpr_batch* b) {
  const int64_t n = b->cfg.n_lanes;
  if (n <= 0) return fail(CPR_E_STATE, "batch has no lockstep lanes (cfg.n_lanes = 0)");
  if (b->cfg.mode != CPR_MODE_GYM) return fail(CPR_E_STATE, "lockstep lanes need CPR_MODE_GYM");
  if (!b->bk_slots.p) {
    HIP_TRY(b->bk_lmem.ensure((size_t)n * (size_t)ev_lane_bytes(b)));
    const size_t sb = b->is_eth ? eth_slot_bytes()
                      : b->cfg.protocol == CPR_PROTO_TAILSTORM ? ts_slot_bytes() : bk_slot_bytes();
    HIP_TRY(b->bk_slots.ensure((size_t)n * sb));
    HIP_TRY(hipMemsetAsync(b->bk_slots.p, 0, (size_t)n * sb, b->ctx->stream));
  }
  return ensure_common_lockstep(b, obs_len_of(b->cfg));
}

// CPR_PROTO_FC16_ENV: one zeroed Fc16Slot per lane, no per-lane region
static int ensure_lockstep_fc16(cpr_batch* b) {
  const int64_t n = b->cfg.n_lanes;
  if (n <= 0) return fail(CPR_E_STATE, "batch has no lockstep lanes (cfg.n_lanes = 0)");
  if (!b->bk_slots.p) {
    HIP_TRY(b->bk_slots.ensure((size_t)n * fc16_slot_bytes()));
    HIP_TRY(hipMemsetAsync(b->bk_slots.p, 0, (size_t)n * fc16_slot_bytes(), b->ctx->stream));
  }
  return ensure_common_lockstep(b, obs_len_of(b->cfg));
}

// CPR_PROTO_GENERIC_NAKAMOTO: one pool of zeroed lane headers and per-lane block regions (the
// regions keep what the allocator gives: a lane writes every byte before it reads it)
static int ensure_lockstep_generic(cpr_batch* b) {
  const int64_t n = b->cfg.n_lanes;
  if (n <= 0) return fail(CPR_E_STATE, "batch has no lockstep lanes (cfg.n_lanes = 0)");
  if (!b->bk_lmem.p) {
    HIP_TRY(b->bk_lmem.ensure(generic_pool_bytes(b->GP, n)));
    HIP_TRY(hipMemsetAsync(b->bk_lmem.p, 0, generic_header_bytes(n), b->ctx->stream));
  }
  return ensure_common_lockstep(b, obs_len_of(b->cfg));
}

static int ensure_lockstep(cpr_batch* b) {
  if (b->fc16_env) return ensure_lockstep_fc16(b);
  if (b->gen_env) return ensure_lockstep_generic(b);
  if (b->is_ev || b->is_eth) return ensure_lockstep_bk(b);
  const int64_t n = b->cfg.n_lanes;
  if (n <= 0) return fail(CPR_E_STATE, "batch has no lockstep lanes (cfg.n_lanes = 0)");
  if (b->cfg.mode != CPR_MODE_GYM) return fail(CPR_E_STATE, "lockstep lanes need CPR_MODE_GYM");
  if (!b->lanes.p) {
    HIP_TRY(b->lanes.ensure((size_t)n * lock_lane_bytes()));
    HIP_TRY(hipMemsetAsync(b->lanes.p, 0, (size_t)n * lock_lane_bytes(), b->ctx->stream));
  }
  if (b->has_rerun && !b->l_alog.p) {
    // lanes leaving the closed form continue on the exact engine: an action log of the
    // episode so far and event-engine lanes handed out on first need and returned at the
    // lane's next reset. Every lane gets a slot and a log of its whole episode when they
    // fit the budgets (kExactSlotBudget of slots: 65,536 lanes of 2,016-step episodes
    // take ~27 GB of the 288 GB; kActionLogBudget of logs), so the lockstep API stays
    // exact for every lane like engine.ml's step (engine.ml:176-249); beyond the budgets
    // (lanes x episode length), a lane that finds no slot keeps the closed form's flags.
    // The slot pool is also capped at a quarter of the device's free memory, and an
    // allocation that fails is retried with half the slots (down to 256) instead of failing
    // the reset: at the gym's delays almost no lane ever leaves the closed form
    constexpr int64_t kExactSlotBudget = 48ll << 30, kActionLogBudget = 4ll << 30;
    const int64_t ms = b->P.max_steps > 0 && b->P.max_steps < (1ll << 30) ? b->P.max_steps
                                                                          : (1 << 14);
    int64_t cap = std::min<int64_t>(ms, kActionLogBudget / n);
    cap = std::max<int64_t>(1, cap);
    b->alog_cap = cap;
    const int64_t eb = std::max<int64_t>(1, b->nak_bytes);
    int64_t slots = std::min<int64_t>(n, std::max<int64_t>(256, kExactSlotBudget / eb));
    size_t free_b = 0, total_b = 0;
    if (hipMemGetInfo(&free_b, &total_b) == hipSuccess)
      slots = std::min<int64_t>(slots, std::max<int64_t>(256, (int64_t)(free_b / 4) / eb));
    slots = std::min<int64_t>(slots, n);
    HIP_TRY(b->l_alog.ensure((size_t)n * (size_t)cap));
    for (;;) {
      const hipError_t e = b->l_emem.ensure((size_t)slots * (size_t)eb);
      if (e == hipSuccess) break;
      (void)hipGetLastError();
      if (slots <= 256) HIP_TRY(e);
      slots = std::max<int64_t>(256, slots / 2);
    }
    b->n_exact_slots = (int32_t)slots;
    HIP_TRY(b->l_eslots.ensure((size_t)b->n_exact_slots * sizeof(eth::EthLane)));
    std::vector<int32_t> stack((size_t)b->n_exact_slots + 1);
    for (int32_t i = 0; i < b->n_exact_slots; i++) stack[i] = i;
    stack[b->n_exact_slots] = b->n_exact_slots;  // stack height: every slot free
    HIP_TRY(b->l_efree.ensure(stack.size() * 4));
    HIP_TRY(hipMemcpy(b->l_efree.p, stack.data(), stack.size() * 4, hipMemcpyHostToDevice));
  }
  HIP_TRY(b->lring.ensure((size_t)n * RING * sizeof(double)));
  HIP_TRY(b->lspill.ensure((size_t)n * b->P.cap * sizeof(double)));
  HIP_TRY(b->lreplay.ensure((size_t)n * REPLAY_BYTES));
  HIP_TRY(b->l_obs.ensure((size_t)n * 4 * sizeof(double)));
  HIP_TRY(b->l_act.ensure((size_t)n * sizeof(int32_t)));
  HIP_TRY(b->l_rew.ensure((size_t)n * sizeof(double)));
  HIP_TRY(b->l_done.ensure((size_t)n));
  HIP_TRY(b->l_mask.ensure((size_t)n));
  HIP_TRY(b->l_eps.ensure((size_t)n * sizeof(uint64_t)));
  HIP_TRY(b->l_info.ensure((size_t)n * (7 * 8 + 3 * 4)));
  return CPR_OK;
}

static LockBuffers lock_buffers(cpr_batch* b) {
  LockBuffers B;
  B.lanes = b->lanes.p;
  B.ring = (double*)b->lring.p;
  B.spill = (double*)b->lspill.p;
  B.replay = (uint8_t*)b->lreplay.p;
  B.alog = (uint8_t*)b->l_alog.p;
  B.alog_cap = b->alog_cap;
  B.emem = (uint8_t*)b->l_emem.p;
  B.elane_bytes = b->nak_bytes;
  B.eslots = b->l_eslots.p;
  B.efree = (int32_t*)b->l_efree.p;
  B.n_slots = b->n_exact_slots;
  return B;
}

// per-lane miner-draw thresholds of a batch with a lane env (null: cfg.alpha's, in the params)
static const uint64_t* lane_thresholds(const cpr_batch* b) {
  return b->has_env ? (const uint64_t*)b->le_lane_t.p : nullptr;
}

// the lanes' step-output buffers (l_obs, l_rew, l_done and the step infos in l_info)
static StepBuffers step_buffers(cpr_batch* b) {
  const int64_t n = b->cfg.n_lanes;
  char* ib = (char*)b->l_info.p;
  StepBuffers sb;
  sb.obs = (double*)b->l_obs.p;
  sb.reward = (double*)b->l_rew.p;
  sb.done = (uint8_t*)b->l_done.p;
  sb.era = (double*)(ib);
  sb.erd = (double*)(ib + n * 8);
  sb.eprog = (double*)(ib + 2 * n * 8);
  sb.ect = (double*)(ib + 3 * n * 8);
  sb.est = (double*)(ib + 4 * n * 8);
  sb.esteps = (int64_t*)(ib + 5 * n * 8);
  sb.eacts = (int64_t*)(ib + 6 * n * 8);
  sb.hh = (int32_t*)(ib + 7 * n * 8);
  sb.hm = (int32_t*)(ib + 7 * n * 8 + n * 4);
  sb.status = (uint32_t*)(ib + 7 * n * 8 + 2 * n * 4);
  return sb;
}

// The device side of one lockstep step, shared by cpr_step and cpr_rollout_net: the
// protocol's step kernel(s) on the device actions `act`, outputs into sb, on the context's
// stream; nothing is copied and nothing waits.
// head_actions: `act` holds indices of the network's action head (the generic env maps them to
// its integer form; every other protocol's actions are head indices anyway)
static int launch_lock_step(cpr_batch* b, const int32_t* act, const StepBuffers& sb,
                            bool head_actions = false) {
  const int64_t n = b->cfg.n_lanes;
  hipStream_t st = b->ctx->stream;
  const double* tabs = (const double*)b->tabs_dev.p;
  const uint64_t* lt = lane_thresholds(b);
  if (b->gen_env)
    HIP_TRY(launch_generic_step(b->GP, b->cfg.seed, b->bk_lmem.p, n, act,
                                head_actions ? b->cfg.k : 0, sb, st, lt));
  else if (b->fc16_env)
    HIP_TRY(launch_fc16_step(b->FP, b->cfg.seed, b->bk_slots.p, n, act, sb, st, lt));
  else if (b->is_eth)
    HIP_TRY(launch_eth_step(b->EP, b->cfg.seed, (uint8_t*)b->bk_lmem.p, b->eth_bytes,
                            b->bk_slots.p, n, act, b->cfg.unit_observation, tabs, b->tab_n, sb,
                            st, lt));
  else if (b->cfg.protocol == CPR_PROTO_BK)
    HIP_TRY(launch_bk_step(b->BP, b->cfg.seed, (uint8_t*)b->bk_lmem.p, b->bk_bytes,
                           b->bk_slots.p, n, act, b->cfg.unit_observation, tabs, b->tab_n, sb,
                           st, lt));
  else if (b->cfg.protocol == CPR_PROTO_TAILSTORM)
    HIP_TRY(launch_ts_step(b->TP, b->cfg.seed, (uint8_t*)b->bk_lmem.p, b->bk_bytes,
                           b->bk_slots.p, n, act, b->cfg.unit_observation, tabs, b->tab_n, sb,
                           st, lt));
  else
  {
    const LockBuffers LB = lock_buffers(b);
    HIP_TRY(launch_step(b->P, b->cfg.seed, LB, n, act, b->cfg.unit_observation, tabs,
                        tabs + b->tab_n, b->tab_n, sb, st, lt));
    HIP_TRY(launch_lock_exact(b->NEP, b->cfg.seed, LB, n, act, b->cfg.unit_observation, tabs,
                              tabs + b->tab_n, b->tab_n, sb, st, lt));
  }
  return CPR_OK;
}

// The device side of a reset, shared by cpr_reset and cpr_rollout_net: the protocol's reset
// kernel with a device mask and device episode ids (either may be null), every lane's
// current observation into obs (device).
// With a lane env the assumption schedule runs first (the event engines simulate up to the
// first interaction inside reset): the masked lanes take their new episode's alpha, and
// out_alpha (optional, device) gets every lane's.
static int launch_lock_reset(cpr_batch* b, const uint8_t* dmask, const uint64_t* deps,
                             double* obs, double* out_alpha = nullptr) {
  const int64_t n = b->cfg.n_lanes;
  hipStream_t st = b->ctx->stream;
  const double* tabs = (const double*)b->tabs_dev.p;
  const uint64_t* lt = lane_thresholds(b);
  if (b->has_env) {
    LaneAssign A;
    A.mask = dmask;
    A.eps = deps;
    A.seed = b->cfg.seed;
    A.n_alpha = b->env.n_alpha;
    A.schedule = b->schedule;
    A.tab_t = (const uint64_t*)b->le_tab_t.p;
    A.tab_a = (const double*)b->le_tab_a.p;
    A.lane_t = (uint64_t*)b->le_lane_t.p;
    A.lane_alpha = (double*)b->le_lane_a.p;
    A.dense_acc = (double*)b->le_acc.p;
    A.out_alpha = out_alpha;
    HIP_TRY(launch_lane_assign(A, n, st));
  }
  if (b->gen_env)
    HIP_TRY(launch_generic_reset(b->GP, b->bk_lmem.p, n, dmask, deps, obs, st, lt));
  else if (b->fc16_env)
    HIP_TRY(launch_fc16_reset(b->FP, b->cfg.seed, b->bk_slots.p, n, dmask, deps, obs, st, lt));
  else if (b->is_eth)
    HIP_TRY(launch_eth_reset(b->EP, b->cfg.seed, (uint8_t*)b->bk_lmem.p, b->eth_bytes,
                             b->bk_slots.p, n, dmask, deps, b->cfg.unit_observation, tabs,
                             b->tab_n, obs, st, lt));
  else if (b->cfg.protocol == CPR_PROTO_BK)
    HIP_TRY(launch_bk_reset(b->BP, b->cfg.seed, (uint8_t*)b->bk_lmem.p, b->bk_bytes,
                            b->bk_slots.p, n, dmask, deps, b->cfg.unit_observation, tabs,
                            b->tab_n, obs, st, lt));
  else if (b->cfg.protocol == CPR_PROTO_TAILSTORM)
    HIP_TRY(launch_ts_reset(b->TP, b->cfg.seed, (uint8_t*)b->bk_lmem.p, b->bk_bytes,
                            b->bk_slots.p, n, dmask, deps, b->cfg.unit_observation, tabs,
                            b->tab_n, obs, st, lt));
  else
    HIP_TRY(launch_reset(b->P, b->NEP, b->cfg.seed, lock_buffers(b), n, dmask, deps,
                         b->cfg.unit_observation, tabs, tabs + b->tab_n, b->tab_n,
                         obs, st, lt));
  return CPR_OK;
}

int cpr_reset(cpr_batch* b, const uint8_t* mask, const uint64_t* eps, double* obs) {
  if (!b || !obs) return fail(CPR_E_INVALID_ARG, "NULL argument");
  CPR_ENTER(b->ctx);
  if (b->cfg.protocol == CPR_PROTO_FC16)
    return fail(CPR_E_UNSUPPORTED, "FC16 runs fused episodes (cpr_run_episodes) only");
  HIP_TRY(hipSetDevice(b->ctx->device));
  int rc = ensure_lockstep(b);
  if (rc) return rc;
  const int64_t n = b->cfg.n_lanes;
  hipStream_t st = b->ctx->stream;
  if (!b->reset_done && mask) {
    for (int64_t i = 0; i < n; i++)
      if (!mask[i]) return fail(CPR_E_STATE, "first reset must include every lane");
  }
  if (b->parked && mask) {
    for (int64_t i = 0; i < n; i++)
      if (!mask[i])
        return fail(CPR_E_STATE, "the reset after cpr_eval_net must include every lane");
  }
  const uint8_t* dmask = nullptr;
  const uint64_t* deps = nullptr;
  if (mask) {
    HIP_TRY(hipMemcpyAsync(b->l_mask.p, mask, (size_t)n, hipMemcpyHostToDevice, st));
    dmask = (const uint8_t*)b->l_mask.p;
  }
  if (eps) {
    HIP_TRY(hipMemcpyAsync(b->l_eps.p, eps, (size_t)n * 8, hipMemcpyHostToDevice, st));
    deps = (const uint64_t*)b->l_eps.p;
  }
  const int ol = obs_len_of(b->cfg);
  rc = launch_lock_reset(b, dmask, deps, (double*)b->l_obs.p);
  if (rc) return rc;
  HIP_TRY(hipMemcpyAsync(obs, b->l_obs.p, (size_t)n * ol * sizeof(double), hipMemcpyDeviceToHost, st));
  HIP_TRY(hipStreamSynchronize(st));
  b->reset_done = true;
  b->parked = false;
  return CPR_OK;
}

int cpr_step(cpr_batch* b, const int32_t* actions, double* obs, double* reward, uint8_t* done,
             cpr_step_info* info) {
  if (!b || !actions || !obs || !reward || !done) return fail(CPR_E_INVALID_ARG, "NULL argument");
  CPR_ENTER(b->ctx);
  if (!b->reset_done) return fail(CPR_E_STATE, "step before reset");
  if (b->parked) return fail(CPR_E_STATE, "step after cpr_eval_net without a reset");
  const int64_t n = b->cfg.n_lanes;
  const int n_act = b->is_eth ? 24 : b->is_ev ? 8 : 4;
  const int ol = obs_len_of(b->cfg);
  // (the generic env takes the reference's integers and clamps them to +-256, mod.rs:214-220)
  for (int64_t i = 0; i < n && !b->gen_env; i++)
    if (actions[i] < 0 || actions[i] >= n_act)
      return fail(CPR_E_INVALID_ARG, "Invalid_argument \"index out of bounds\" (action)");
  HIP_TRY(hipSetDevice(b->ctx->device));
  hipStream_t st = b->ctx->stream;
  HIP_TRY(hipMemcpyAsync(b->l_act.p, actions, (size_t)n * 4, hipMemcpyHostToDevice, st));
  const StepBuffers sb = step_buffers(b);
  int rc = launch_lock_step(b, (const int32_t*)b->l_act.p, sb);
  if (rc) return rc;
  HIP_TRY(hipMemcpyAsync(obs, sb.obs, (size_t)n * ol * 8, hipMemcpyDeviceToHost, st));
  HIP_TRY(hipMemcpyAsync(reward, sb.reward, (size_t)n * 8, hipMemcpyDeviceToHost, st));
  HIP_TRY(hipMemcpyAsync(done, sb.done, (size_t)n, hipMemcpyDeviceToHost, st));
  if (info) {
    struct {
      void* dst;
      void* src;
      size_t sz;
    } cp[] = {{info->episode_reward_attacker, sb.era, 8},  {info->episode_reward_defender, sb.erd, 8},
              {info->episode_progress, sb.eprog, 8},       {info->episode_chain_time, sb.ect, 8},
              {info->episode_sim_time, sb.est, 8},         {info->episode_n_steps, sb.esteps, 8},
              {info->episode_n_activations, sb.eacts, 8},  {info->head_height, sb.hh, 4},
              {info->head_miner, sb.hm, 4},                {info->status, sb.status, 4}};
    for (auto& x : cp)
      if (x.dst) HIP_TRY(hipMemcpyAsync(x.dst, x.src, (size_t)n * x.sz, hipMemcpyDeviceToHost, st));
  }
  HIP_TRY(hipStreamSynchronize(st));
  return CPR_OK;
}

int cpr_observe_fields(cpr_batch* b, int32_t* fields) {
  if (!b || !fields) return fail(CPR_E_INVALID_ARG, "NULL argument");
  CPR_ENTER(b->ctx);
  if (!b->reset_done) return fail(CPR_E_STATE, "observe before reset");
  const int64_t n = b->cfg.n_lanes;
  HIP_TRY(hipSetDevice(b->ctx->device));
  hipStream_t st = b->ctx->stream;
  const size_t per = (size_t)(b->gen_env ? 7 : obs_len_of(b->cfg)) * 4;
  DevBuf tmp;
  HIP_TRY(tmp.ensure((size_t)n * per));
  if (b->gen_env)
    HIP_TRY(launch_generic_observe_fields(b->GP, b->bk_lmem.p, n, (int32_t*)tmp.p, st));
  else if (b->fc16_env)
    HIP_TRY(launch_fc16_observe_fields(b->bk_slots.p, n, (int32_t*)tmp.p, st));
  else if (b->is_eth)
    HIP_TRY(launch_eth_observe_fields(b->EP, (uint8_t*)b->bk_lmem.p, b->eth_bytes, b->bk_slots.p,
                                      n, (int32_t*)tmp.p, st));
  else if (b->cfg.protocol == CPR_PROTO_BK)
    HIP_TRY(launch_bk_observe_fields(b->BP, (uint8_t*)b->bk_lmem.p, b->bk_bytes, b->bk_slots.p,
                                     n, (int32_t*)tmp.p, st));
  else if (b->cfg.protocol == CPR_PROTO_TAILSTORM)
    HIP_TRY(launch_ts_observe_fields(b->TP, (uint8_t*)b->bk_lmem.p, b->bk_bytes, b->bk_slots.p,
                                     n, (int32_t*)tmp.p, st));
  else
    HIP_TRY(launch_observe_fields(b->NEP, lock_buffers(b), n, (int32_t*)tmp.p, st,
                                  lane_thresholds(b)));
  HIP_TRY(hipMemcpyAsync(fields, tmp.p, (size_t)n * per, hipMemcpyDeviceToHost, st));
  HIP_TRY(hipStreamSynchronize(st));
  tmp.release();
  return CPR_OK;
}

int cpr_policy_actions(cpr_batch* b, int32_t policy, const double* obs, int64_t n,
                       int32_t* actions) {
  if (!b || !obs || !actions) return fail(CPR_E_INVALID_ARG, "NULL argument");
  CPR_ENTER(b->ctx);
  if (b->fc16_env)
    return fail(CPR_E_UNSUPPORTED, "FC16 env: the built-in policies read (a, h, fork) in the "
                                   "fused episodes (cpr_run_episodes), not encoded observations");
  if (b->gen_env)
    return fail(CPR_E_UNSUPPORTED, "generic env: no built-in policies on encoded observations "
                                   "(honest play reads cpr_observe_fields)");
  if (b->cfg.protocol == CPR_PROTO_TAILSTORM) {
    if (policy < 0 || policy > CPR_TS_POLICY_TABLE)
      return fail(CPR_E_INVALID_ARG, "unknown policy");
    if (policy == CPR_TS_POLICY_TABLE && b->table_host.empty())
      return fail(CPR_E_INVALID_ARG, "batch has no policy table");
    if (n <= 0) return CPR_OK;
    HIP_TRY(hipSetDevice(b->ctx->device));
    hipStream_t st = b->ctx->stream;
    DevBuf& o = b->pol_obs;
    DevBuf& a = b->pol_act;
    HIP_TRY(o.ensure((size_t)n * 80));
    HIP_TRY(a.ensure((size_t)n * 4));
    HIP_TRY(hipMemcpyAsync(o.p, obs, (size_t)n * 80, hipMemcpyHostToDevice, st));
    HIP_TRY(launch_ts_policy(policy, b->cfg.k, b->cfg.unit_observation, (const double*)o.p, n,
                             (const uint8_t*)b->table_dev.p, b->cfg.policy_table_dim,
                             (int32_t*)a.p, st));
    HIP_TRY(hipMemcpyAsync(actions, a.p, (size_t)n * 4, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    return CPR_OK;
  }
  if (b->cfg.protocol == CPR_PROTO_BK) {
    if (policy < 0 || policy > CPR_BK_POLICY_TABLE) return fail(CPR_E_INVALID_ARG, "unknown policy");
    if (policy == CPR_BK_POLICY_TABLE && b->table_host.empty())
      return fail(CPR_E_INVALID_ARG, "batch has no policy table");
    if (n <= 0) return CPR_OK;
    HIP_TRY(hipSetDevice(b->ctx->device));
    hipStream_t st = b->ctx->stream;
    DevBuf& o = b->pol_obs;
    DevBuf& a = b->pol_act;
    HIP_TRY(o.ensure((size_t)n * 64));
    HIP_TRY(a.ensure((size_t)n * 4));
    HIP_TRY(hipMemcpyAsync(o.p, obs, (size_t)n * 64, hipMemcpyHostToDevice, st));
    bk::BkParams P = b->BP;
    P.policy = policy;
    HIP_TRY(launch_bk_policy(P, b->cfg.unit_observation, (const double*)o.p, n, (int32_t*)a.p, st));
    HIP_TRY(hipMemcpyAsync(actions, a.p, (size_t)n * 4, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    return CPR_OK;
  }
  if (b->is_eth) {
    if (policy < 0 || policy > CPR_ETH_POLICY_TABLE)
      return fail(CPR_E_INVALID_ARG, "unknown policy");
    if (policy == CPR_ETH_POLICY_TABLE && b->table_host.empty())
      return fail(CPR_E_INVALID_ARG, "batch has no policy table");
    if (n <= 0) return CPR_OK;
    HIP_TRY(hipSetDevice(b->ctx->device));
    hipStream_t st = b->ctx->stream;
    DevBuf& o = b->pol_obs;
    DevBuf& a = b->pol_act;
    HIP_TRY(o.ensure((size_t)n * 80));
    HIP_TRY(a.ensure((size_t)n * 4));
    HIP_TRY(hipMemcpyAsync(o.p, obs, (size_t)n * 80, hipMemcpyHostToDevice, st));
    HIP_TRY(launch_eth_policy(policy, b->cfg.unit_observation, (const double*)o.p, n,
                              (const uint8_t*)b->table_dev.p, b->cfg.policy_table_dim,
                              (int32_t*)a.p, st));
    HIP_TRY(hipMemcpyAsync(actions, a.p, (size_t)n * 4, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    return CPR_OK;
  }
  if (b->cfg.protocol != CPR_PROTO_NAKAMOTO)
    return fail(CPR_E_UNSUPPORTED, "policy evaluation on encoded observations");
  if (policy < 0 || policy > CPR_POLICY_TABLE) return fail(CPR_E_INVALID_ARG, "unknown policy");
  if (policy == CPR_POLICY_TABLE && b->table_host.empty())
    return fail(CPR_E_INVALID_ARG, "batch has no policy table");
  if (n <= 0) return CPR_OK;
  HIP_TRY(hipSetDevice(b->ctx->device));
  hipStream_t st = b->ctx->stream;
  DevBuf& o = b->pol_obs;
  DevBuf& a = b->pol_act;
  HIP_TRY(o.ensure((size_t)n * 32));
  HIP_TRY(a.ensure((size_t)n * 4));
  HIP_TRY(hipMemcpyAsync(o.p, obs, (size_t)n * 32, hipMemcpyHostToDevice, st));
  HIP_TRY(launch_policy(policy, b->cfg.unit_observation, (const double*)o.p, n,
                        (const uint8_t*)b->table_dev.p, b->cfg.policy_table_dim, (int32_t*)a.p,
                        st));
  HIP_TRY(hipMemcpyAsync(actions, a.p, (size_t)n * 4, hipMemcpyDeviceToHost, st));
  HIP_TRY(hipStreamSynchronize(st));
  return CPR_OK;
}

// ssz_tools.ml:64-73 ranges; nakamoto_ssz.ml:43-61
int cpr_observation_spec(cpr_batch* b, int32_t* obs_len, int32_t* n_actions, double* low,
                         double* high) {
  if (!b) return fail(CPR_E_INVALID_ARG, "NULL argument");
  CPR_ENTER(b->ctx);
  const double inf = __builtin_inf();
  if (b->gen_env) {
    // mod.rs:913-925 with nakamoto.rs:106-112; the head of 1 + 2K actions (cpr_hip.h)
    if (obs_len) *obs_len = 5;
    if (n_actions) *n_actions = 1 + 2 * b->cfg.k;
    const double lo[5] = {0.0, 0.0, 0.0, -1.0, 0.0};
    const double hi[5] = {(double)__FLT_MAX__, (double)__FLT_MAX__, 1.0, 0.0, 1.0};
    for (int i = 0; i < 5; i++) {
      if (low) low[i] = lo[i];
      if (high) high[i] = hi[i];
    }
    return CPR_OK;
  }
  if (b->is_fc16) {
    // fc16.rs:61-73: (a, h, fork index) each mapped x -> x / (1 + x); at most 4 actions
    if (obs_len) *obs_len = 3;
    if (n_actions) *n_actions = 4;
    for (int i = 0; i < 3; i++) {
      if (low) low[i] = 0.0;
      if (high) high[i] = 1.0;
    }
    return CPR_OK;
  }
  if (b->cfg.protocol == CPR_PROTO_TAILSTORM) {
    // tailstorm_ssz.ml:41-79: 10 fields (diff signed, event discrete), Action8
    if (obs_len) *obs_len = 10;
    if (n_actions) *n_actions = 8;
    for (int i = 0; i < 10; i++) {
      double lo = 0.0, hi = 1.0;
      if (!b->cfg.unit_observation) {
        lo = i == 2 ? -inf : 0.0;
        hi = i == 9 ? 2.0 : inf;
      }
      if (low) low[i] = lo;
      if (high) high[i] = hi;
    }
    return CPR_OK;
  }
  if (b->cfg.protocol == CPR_PROTO_BK) {
    // bk_ssz.ml:37-74 normalizers; ssz_tools.ml:64-74 ranges (raw Bool range is (0, 0))
    if (obs_len) *obs_len = 8;
    if (n_actions) *n_actions = 8;
    for (int i = 0; i < 8; i++) {
      double lo = 0.0, hi = 1.0;
      if (!b->cfg.unit_observation) {
        lo = i == 2 ? -inf : 0.0;
        hi = i == 6 ? 0.0 : (i == 7 ? 2.0 : inf);
      }
      if (low) low[i] = lo;
      if (high) high[i] = hi;
    }
    return CPR_OK;
  }
  if (b->cfg.protocol == CPR_PROTO_ETHEREUM) {
    // ethereum_ssz.ml:47-80: 10 fields (diff_* signed, event discrete), 24 actions
    if (obs_len) *obs_len = 10;
    if (n_actions) *n_actions = 24;
    for (int i = 0; i < 10; i++) {
      const bool sgn = i == 4 || i == 5;
      double lo = 0.0, hi = 1.0;
      if (!b->cfg.unit_observation && i != 9) {
        lo = sgn ? -inf : 0.0;
        hi = inf;
      }
      if (low) low[i] = lo;
      if (high) high[i] = hi;
    }
    return CPR_OK;
  }
  if (obs_len) *obs_len = 4;
  if (n_actions) *n_actions = 4;
  if (b->cfg.unit_observation) {
    for (int i = 0; i < 4; i++) {
      if (low) low[i] = 0.0;
      if (high) high[i] = 1.0;
    }
  } else {
    const double lo[4] = {0.0, 0.0, -inf, 0.0}, hi[4] = {inf, inf, inf, 1.0};
    for (int i = 0; i < 4; i++) {
      if (low) low[i] = lo[i];
      if (high) high[i] = hi[i];
    }
  }
  return CPR_OK;
}

// Collection.add prepends (collection.ml:13): registry order is the reverse of the adds
// in nakamoto_ssz.ml:342-350
static const char* kNames[4] = {"sapirshtein-2016-sm1", "eyal-sirer-2014", "simple", "honest"};
static const int32_t kIds[4] = {CPR_POLICY_SAPIRSHTEIN_2016_SM1, CPR_POLICY_EYAL_SIRER_2014,
                                CPR_POLICY_SIMPLE, CPR_POLICY_HONEST};

// ethereum_ssz.ml:523-538, same reversal
static const char* kEthNames[5] = {"fn19pkel", "fn19", "selfish_discard", "selfish_release",
                                   "honest"};
static const int32_t kEthIds[5] = {CPR_ETH_POLICY_FN19PKEL, CPR_ETH_POLICY_FN19,
                                   CPR_ETH_POLICY_SELFISH_DISCARD,
                                   CPR_ETH_POLICY_SELFISH_RELEASE, CPR_ETH_POLICY_HONEST};

// bk_ssz.ml:404-415, same reversal
static const char* kBkNames[4] = {"avoid-loss", "minor-delay", "get-ahead", "honest"};
static const int32_t kBkIds[4] = {CPR_BK_POLICY_AVOID_LOSS, CPR_BK_POLICY_MINOR_DELAY,
                                  CPR_BK_POLICY_GET_AHEAD, CPR_BK_POLICY_HONEST};

// tailstorm_ssz.ml:449-472, same reversal
static const char* kTsNames[7] = {"long-delay", "avoid-loss-b", "avoid-loss-a", "avoid-loss",
                                  "minor-delay", "get-ahead", "honest"};
static const int32_t kTsIds[7] = {CPR_TS_POLICY_LONG_DELAY, CPR_TS_POLICY_AVOID_LOSS_B,
                                  CPR_TS_POLICY_AVOID_LOSS_A, CPR_TS_POLICY_AVOID_LOSS,
                                  CPR_TS_POLICY_MINOR_DELAY, CPR_TS_POLICY_GET_AHEAD,
                                  CPR_TS_POLICY_HONEST};

int cpr_policy_count(int32_t protocol) {
  switch (protocol) {
    case CPR_PROTO_NAKAMOTO: return 4;
    case CPR_PROTO_ETHEREUM: return 5;
    case CPR_PROTO_BK: return 4;
    case CPR_PROTO_TAILSTORM: return 7;
    default: return 0;
  }
}

const char* cpr_policy_name(int32_t protocol, int32_t index, int32_t* policy_id) {
  if (index < 0 || index >= cpr_policy_count(protocol)) {
    g_err = "no such policy";
    return nullptr;
  }
  if (protocol == CPR_PROTO_ETHEREUM) {
    if (policy_id) *policy_id = kEthIds[index];
    return kEthNames[index];
  }
  if (protocol == CPR_PROTO_BK) {
    if (policy_id) *policy_id = kBkIds[index];
    return kBkNames[index];
  }
  if (protocol == CPR_PROTO_TAILSTORM) {
    if (policy_id) *policy_id = kTsIds[index];
    return kTsNames[index];
  }
  if (policy_id) *policy_id = kIds[index];
  return kNames[index];
}

// cpr_rollout over the Nakamoto closed-form lanes: rounds of the closed-form pass and the
// exact pass (kernels.hip k_nak_rollout, k_nak_rollout_exact) until no lane has steps left.
// The lanes-left word sits behind the device summary and comes back in the same copy. Every
// round advances each unfinished lane by at least one step, so n_steps + 1 rounds always
// suffice: past that bound the call fails instead of spinning. On success the stream is idle
// and *out holds the call's summary.
static int nak_rollout_rounds(cpr_batch* b, int64_t n_steps, double* obs, double* reward,
                              uint8_t* done, cpr_summary* out) {
  static_assert(sizeof(cpr_summary) % 8 == 0, "the lanes-left word follows the summary");
  struct {
    cpr_summary s;
    unsigned long long left;
  } host;
  const int64_t n = b->cfg.n_lanes;
  hipStream_t st = b->ctx->stream;
  HIP_TRY(b->l_cur.ensure((size_t)n * sizeof(int64_t)));
  HIP_TRY(b->l_rsum.ensure(sizeof(host)));
  HIP_TRY(hipMemsetAsync(b->l_cur.p, 0, (size_t)n * sizeof(int64_t), st));
  HIP_TRY(hipMemsetAsync(b->l_rsum.p, 0, sizeof(host), st));
  RollBuffers R;
  R.cursor = (int64_t*)b->l_cur.p;
  R.sum = (cpr_summary*)b->l_rsum.p;
  R.left = (unsigned long long*)((char*)b->l_rsum.p + sizeof(cpr_summary));
  R.obs = obs;
  R.reward = reward;
  R.done = done;
  R.n_steps = n_steps;
  const LockBuffers LB = lock_buffers(b);
  const double* tabs = (const double*)b->tabs_dev.p;
  for (int64_t round = 0;; ++round) {
    if (round > n_steps)
      return fail(CPR_E_STATE, "cpr_rollout: lanes still have steps left after n_steps + 1 "
                               "rounds of the closed-form and exact passes");
    if (round > 0) HIP_TRY(hipMemsetAsync(R.left, 0, sizeof(unsigned long long), st));
    HIP_TRY(launch_nak_rollout(b->P, b->cfg.seed, LB, n, R, b->cfg.unit_observation, tabs,
                               tabs + b->tab_n, b->tab_n, st));
    HIP_TRY(launch_nak_rollout_exact(b->P, b->NEP, b->cfg.seed, LB, n, R,
                                     b->cfg.unit_observation, tabs, tabs + b->tab_n, b->tab_n,
                                     st));
    HIP_TRY(hipMemcpyAsync(&host, b->l_rsum.p, sizeof(host), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    if (host.left == 0) break;
  }
  *out = host.s;
  return CPR_OK;
}

int cpr_rollout(cpr_batch* b, int64_t n_steps, double* obs, double* reward, uint8_t* done,
                int outputs_on_device, cpr_summary* summary) {
  if (!b || !summary) return fail(CPR_E_INVALID_ARG, "NULL argument");
  CPR_ENTER(b->ctx);
  if (b->fc16_env)
    return fail(CPR_E_UNSUPPORTED, "FC16 env: the built-in policies run as fused episodes "
                                   "(cpr_run_episodes); rollouts take a network (cpr_rollout_net)");
  if (b->gen_env)
    return fail(CPR_E_UNSUPPORTED, "generic env: no built-in policies; rollouts take a network "
                                   "(cpr_rollout_net)");
  if (b->env_table)
    return fail(CPR_E_UNSUPPORTED, "cpr_rollout (built-in policies) runs every lane at cfg.alpha; "
                                   "this batch has an alpha table (cpr_lane_env_set)");
  if (b->parked) return fail(CPR_E_STATE, "rollout after cpr_eval_net without a reset");
  const bool is_nak = !b->is_ev && !b->is_eth;
  if (is_nak) {
    // the closed-form lane's rollout (k_nak_rollout): the gym's networks, policies the lane
    // can evaluate on its own observation
    if (b->cfg.protocol != CPR_PROTO_NAKAMOTO)
      return fail(CPR_E_UNSUPPORTED,
                  "cpr_rollout is implemented for Nakamoto, Ethereum, B_k and Tailstorm");
    if (b->nak_ev || (b->cfg.network != CPR_NET_SELFISH_MINING &&
                      b->cfg.network != CPR_NET_ABSTRACT_GAMMA))
      return fail(CPR_E_UNSUPPORTED,
                  "cpr_rollout (Nakamoto): selfish-mining and abstract-gamma networks only");
    if (b->cfg.policy < CPR_POLICY_HONEST || b->cfg.policy > CPR_POLICY_TABLE)
      return fail(CPR_E_UNSUPPORTED,
                  "cpr_rollout (Nakamoto): built-in policies and CPR_POLICY_TABLE only");
  }
  if (n_steps <= 0) return CPR_OK;
  HIP_TRY(hipSetDevice(b->ctx->device));
  int rc = ensure_lockstep(b);
  if (rc) return rc;
  hipStream_t st = b->ctx->stream;
  HIP_TRY(b->summary.ensure(sizeof(cpr_summary)));
  HIP_TRY(hipMemsetAsync(b->summary.p, 0, sizeof(cpr_summary), st));
  if (!b->ev0) {
    HIP_TRY(hipEventCreate(&b->ev0));
    HIP_TRY(hipEventCreate(&b->ev1));
  }
  const int64_t cells = n_steps * b->cfg.n_lanes;
  const int ol = obs_len_of(b->cfg);
  double* obs_dev = obs;
  double* reward_dev = reward;
  uint8_t* done_dev = done;
  DevBuf so, sr, sd;
  if (!outputs_on_device) {
    if (obs) {
      HIP_TRY(so.ensure((size_t)cells * ol * 8));
      obs_dev = (double*)so.p;
    }
    if (reward) {
      HIP_TRY(sr.ensure((size_t)cells * 8));
      reward_dev = (double*)sr.p;
    }
    if (done) {
      HIP_TRY(sd.ensure((size_t)cells));
      done_dev = (uint8_t*)sd.p;
    }
  }
  const double* tabs = (const double*)b->tabs_dev.p;
  HIP_TRY(hipEventRecord(b->ev0, st));
  cpr_summary s;
  if (is_nak) {
    rc = nak_rollout_rounds(b, n_steps, obs_dev, reward_dev, done_dev, &s);
    if (rc) return rc;
  } else if (b->is_eth)
    HIP_TRY(launch_eth_rollout(b->EP, b->cfg.seed, (uint8_t*)b->bk_lmem.p, b->eth_bytes,
                               b->bk_slots.p, b->cfg.n_lanes, n_steps, b->cfg.unit_observation,
                               tabs, b->tab_n, obs_dev, reward_dev, done_dev,
                               (cpr_summary*)b->summary.p, st));
  else if (b->cfg.protocol == CPR_PROTO_TAILSTORM)
    HIP_TRY(launch_ts_rollout(b->TP, b->cfg.seed, (uint8_t*)b->bk_lmem.p, b->bk_bytes,
                              b->bk_slots.p, b->cfg.n_lanes, n_steps, b->cfg.unit_observation,
                              tabs, b->tab_n, obs_dev, reward_dev, done_dev,
                              (cpr_summary*)b->summary.p, st));
  else
    HIP_TRY(launch_bk_rollout(b->BP, b->cfg.seed, (uint8_t*)b->bk_lmem.p, b->bk_bytes,
                              b->bk_slots.p, b->cfg.n_lanes, n_steps, b->cfg.unit_observation,
                              tabs, b->tab_n, obs_dev, reward_dev, done_dev,
                              (cpr_summary*)b->summary.p, st));
  HIP_TRY(hipEventRecord(b->ev1, st));
  if (!is_nak)
    HIP_TRY(hipMemcpyAsync(&s, b->summary.p, sizeof(s), hipMemcpyDeviceToHost, st));
  if (!outputs_on_device) {
    if (obs) HIP_TRY(hipMemcpyAsync(obs, obs_dev, (size_t)cells * ol * 8, hipMemcpyDeviceToHost, st));
    if (reward) HIP_TRY(hipMemcpyAsync(reward, reward_dev, (size_t)cells * 8, hipMemcpyDeviceToHost, st));
    if (done) HIP_TRY(hipMemcpyAsync(done, done_dev, (size_t)cells, hipMemcpyDeviceToHost, st));
  }
  HIP_TRY(hipStreamSynchronize(st));
  so.release();
  sr.release();
  sd.release();
  float ms = 0.f;
  HIP_TRY(hipEventElapsedTime(&ms, b->ev0, b->ev1));
  b->last_ms = ms;
  b->last_acts = s.activations;
  b->reset_done = true;
  // rollout lanes are the batch's n_lanes (one thread each, 256-thread workgroups); the
  // resident figure is the fused-episode kernel's occupancy of the same lane
  b->last_lanes = b->cfg.n_lanes;
  b->last_resident = (int64_t)b->ctx->cus * 256 *
                     (is_nak ? nak_rollout_blocks_per_cu() : b->is_eth ? eth_blocks_per_cu()
                                : (b->cfg.protocol == CPR_PROTO_TAILSTORM ? ts_blocks_per_cu()
                                                                          : bk_blocks_per_cu()));
  summary->episodes += s.episodes;
  summary->steps += s.steps;
  summary->activations += s.activations;
  summary->reward_attacker_fx += s.reward_attacker_fx;
  summary->reward_defender_fx += s.reward_defender_fx;
  summary->progress_fx += s.progress_fx;
  summary->rel_revenue_fx += s.rel_revenue_fx;
  summary->rel_revenue_sq_fx += s.rel_revenue_sq_fx;
  summary->orphans += s.orphans;
  summary->status_tie += s.status_tie;
  summary->status_overlap += s.status_overlap;
  summary->status_other += s.status_other;
  summary->invalid += s.invalid;
  for (int i = 0; i < CPR_HIST_BINS; i++) summary->hist[i] += s.hist[i];
  return CPR_OK;
}

// ---------------------------------------------------------------- neural-network policies

// Q-learning's view of a new network b->pn (cpr_dqn_init, cpr_policy_net_set / _copy on a batch
// with a ring): the target becomes a copy of the weights in the same padded layout, the
// gradient buffer is zero (its vf part stays so), the update count starts over
static int dqn_target_reset(cpr_batch* b) {
  hipStream_t st = b->ctx->stream;
  const size_t bytes = (size_t)b->pn_total * sizeof(float);
  HIP_TRY(hipStreamSynchronize(st));  // a kernel may still be reading the previous buffers
  HIP_TRY(b->dq_tw.ensure(bytes));
  HIP_TRY(b->dq_grad.ensure(bytes));
  HIP_TRY(hipMemcpyAsync(b->dq_tw.p, b->pn_w.p, bytes, hipMemcpyDeviceToDevice, st));
  HIP_TRY(hipMemsetAsync(b->dq_grad.p, 0, b->dq_grad.bytes, st));
  b->dq_tn = b->pn;
  const float* from = (const float*)b->pn_w.p;
  const float* to = (const float*)b->dq_tw.p;
  for (PolLayer* Ls : {b->dq_tn.pi, b->dq_tn.vf})
    for (int l = 0; l <= b->pn.depth; l++) {
      Ls[l].W = to + (Ls[l].W - from);
      Ls[l].b = to + (Ls[l].b - from);
    }
  b->dq_updates = 0;
  return CPR_OK;
}

int cpr_policy_net_set(cpr_batch* b, const cpr_policy_net* net) {
  if (!b || !net) return fail(CPR_E_INVALID_ARG, "NULL argument");
  CPR_ENTER(b->ctx);
  if (b->cfg.protocol == CPR_PROTO_FC16)
    return fail(CPR_E_UNSUPPORTED, "FC16 runs fused episodes (cpr_run_episodes) only");
  if (b->cfg.n_lanes <= 0 || b->cfg.mode != CPR_MODE_GYM)
    return fail(CPR_E_UNSUPPORTED, "a policy network needs lockstep lanes (CPR_MODE_GYM, "
                                   "cfg.n_lanes > 0)");
  if (net->depth < 1 || net->depth > kPolMaxDepth)
    return fail(CPR_E_INVALID_ARG, "policy net: depth must be in 1..4");
  for (int32_t w : {net->width_pi, net->width_vf})
    if (w < 16 || w > kPolMaxWidth || w % 16 != 0)
      return fail(CPR_E_INVALID_ARG, "policy net: width must be a multiple of 16 in [16, 512]");
  if (net->n_extra < 0 || net->n_extra > kPolMaxExtra)
    return fail(CPR_E_INVALID_ARG, "policy net: n_extra must be in 0..8");
  for (int i = 0; i < net->n_extra; i++)
    if (!std::isfinite(net->extra[i]))
      return fail(CPR_E_INVALID_ARG, "policy net: non-finite extra feature");
  if (b->has_env && b->env.alpha_column >= net->n_extra)
    return fail(CPR_E_INVALID_ARG, "policy net: n_extra does not reach the lane env's "
                                   "alpha_column (cpr_lane_env_set)");
  int32_t ol = 0, na = 0;
  int rc = cpr_observation_spec(b, &ol, &na, nullptr, nullptr);
  if (rc) return rc;
  if (ol + net->n_extra > kPolInStride || na > kPolMaxActions)
    return fail(CPR_E_UNSUPPORTED, "policy net: input or action head wider than the kernel's tile");
  HIP_TRY(hipSetDevice(b->ctx->device));
  // the LDS a workgroup's tile needs, checked here so that no launch can exceed the device
  const int64_t lds = policy_lds_bytes(net->depth, net->width_pi, net->width_vf);
  if (lds > policy_lds_limit())
    return fail(CPR_E_UNSUPPORTED,
                "policy net: depth " + std::to_string(net->depth) + ", width " +
                    std::to_string(std::max(net->width_pi, net->width_vf)) + " needs " +
                    std::to_string(lds) + " B of LDS per workgroup, the device has " +
                    std::to_string(policy_lds_limit()));
  // one host image of every array, then one upload; offsets in floats
  struct Arr {
    const float* src;
    int64_t count;
    const float** dst;
  };
  PolNet N = {};
  N.obs_len = ol;
  N.n_extra = net->n_extra;
  N.depth = net->depth;
  N.n_actions = na;
  N.width_pi = net->width_pi;
  N.width_vf = net->width_vf;
  for (int i = 0; i < net->n_extra; i++) N.extra[i] = net->extra[i];
  std::vector<Arr> arrs;
  for (int trunk = 0; trunk < 2; trunk++) {
    PolLayer* Ls = trunk == 0 ? N.pi : N.vf;
    const int32_t width = trunk == 0 ? net->width_pi : net->width_vf;
    const float* const* ws = trunk == 0 ? net->pi_w : net->vf_w;
    const float* const* bs = trunk == 0 ? net->pi_b : net->vf_b;
    for (int l = 0; l <= net->depth; l++) {
      const bool head = l == net->depth;
      Ls[l].n_in = l == 0 ? ol + net->n_extra : width;
      Ls[l].n_out = head ? (trunk == 0 ? na : 1) : width;
      const float* w = head ? (trunk == 0 ? net->pi_head_w : net->vf_head_w) : ws[l];
      const float* bias = head ? (trunk == 0 ? net->pi_head_b : net->vf_head_b) : bs[l];
      if (!w || !bias) return fail(CPR_E_INVALID_ARG, "policy net: NULL weight or bias array");
      arrs.push_back({w, (int64_t)Ls[l].n_in * Ls[l].n_out, &Ls[l].W});
      arrs.push_back({bias, (int64_t)Ls[l].n_out, &Ls[l].b});
    }
  }
  std::vector<float> host;
  std::vector<int64_t> offs;
  for (const Arr& a : arrs) {
    offs.push_back((int64_t)host.size());
    for (int64_t i = 0; i < a.count; i++) {
      if (!std::isfinite(a.src[i]))
        return fail(CPR_E_INVALID_ARG, "policy net: non-finite weight or bias");
      host.push_back(a.src[i]);
    }
    while (host.size() % 4) host.push_back(0.f);
  }
  // a forward of the previous network may still be reading the buffer
  HIP_TRY(hipStreamSynchronize(b->ctx->stream));
  HIP_TRY(b->pn_w.ensure(host.size() * sizeof(float)));
  HIP_TRY(hipMemcpy(b->pn_w.p, host.data(), host.size() * sizeof(float), hipMemcpyHostToDevice));
  for (size_t i = 0; i < arrs.size(); i++) *arrs[i].dst = (const float*)b->pn_w.p + offs[i];
  // the learner's view of the buffer; Adam starts over with a new network
  b->pn_off = offs;
  b->pn_cnt.clear();
  for (const Arr& a : arrs) b->pn_cnt.push_back(a.count);
  b->pn_total = (int64_t)host.size();
  b->ppo_t = 0;
  b->ppo_updates = 0;
  if (b->pp_m.p) HIP_TRY(hipMemsetAsync(b->pp_m.p, 0, b->pp_m.bytes, b->ctx->stream));
  if (b->pp_v.p) HIP_TRY(hipMemsetAsync(b->pp_v.p, 0, b->pp_v.bytes, b->ctx->stream));
  b->pp_part.release();  // its zeroed padding stood where the previous network's was
  b->pn = N;
  b->has_net = true;
  if (b->dq_ready) return dqn_target_reset(b);
  return CPR_OK;
}

int cpr_policy_net_forward(cpr_batch* b, const double* obs, int64_t n, int deterministic,
                           uint64_t episode0, int32_t* actions, double* logp, double* value,
                           float* logits) {
  if (!b || !obs) return fail(CPR_E_INVALID_ARG, "NULL argument");
  CPR_ENTER(b->ctx);
  if (!b->has_net) return fail(CPR_E_STATE, "no policy network set (cpr_policy_net_set)");
  if (n < 1) return fail(CPR_E_INVALID_ARG, "policy net forward: n must be >= 1");
  HIP_TRY(hipSetDevice(b->ctx->device));
  hipStream_t st = b->ctx->stream;
  const int ol = b->pn.obs_len, na = b->pn.n_actions;
  const size_t o_act = 0, o_logp = align256((size_t)n * 4), o_val = o_logp + align256((size_t)n * 8),
               o_lg = o_val + align256((size_t)n * 8), total = o_lg + (size_t)n * na * 4;
  HIP_TRY(b->pn_in.ensure((size_t)n * ol * 8));
  HIP_TRY(b->pn_out.ensure(total));
  char* ob = (char*)b->pn_out.p;
  HIP_TRY(hipMemcpyAsync(b->pn_in.p, obs, (size_t)n * ol * 8, hipMemcpyHostToDevice, st));
  PolIO io = {};
  io.obs = (const double*)b->pn_in.p;
  io.n = n;
  io.deterministic = deterministic ? 1 : 0;
  io.seed = b->cfg.seed;
  io.episode0 = episode0;
  io.action = actions ? (int32_t*)(ob + o_act) : nullptr;
  io.logp = logp ? (double*)(ob + o_logp) : nullptr;
  io.value = value ? (double*)(ob + o_val) : nullptr;
  io.logits = logits ? (float*)(ob + o_lg) : nullptr;
  if (!b->ev0) {
    HIP_TRY(hipEventCreate(&b->ev0));
    HIP_TRY(hipEventCreate(&b->ev1));
  }
  HIP_TRY(hipEventRecord(b->ev0, st));
  HIP_TRY(launch_policy_forward(b->pn, io, st));
  HIP_TRY(hipEventRecord(b->ev1, st));
  if (actions) HIP_TRY(hipMemcpyAsync(actions, io.action, (size_t)n * 4, hipMemcpyDeviceToHost, st));
  if (logp) HIP_TRY(hipMemcpyAsync(logp, io.logp, (size_t)n * 8, hipMemcpyDeviceToHost, st));
  if (value) HIP_TRY(hipMemcpyAsync(value, io.value, (size_t)n * 8, hipMemcpyDeviceToHost, st));
  if (logits)
    HIP_TRY(hipMemcpyAsync(logits, io.logits, (size_t)n * na * 4, hipMemcpyDeviceToHost, st));
  HIP_TRY(hipStreamSynchronize(st));
  float ms = 0.f;  // cpr_last_launch: the forward kernel alone
  HIP_TRY(hipEventElapsedTime(&ms, b->ev0, b->ev1));
  b->last_ms = ms;
  b->last_acts = 0;
  b->async_launch = false;
  return CPR_OK;
}

// where the lanes stand, from the protocol's own lane state
static int launch_lane_cursor(cpr_batch* b, const LaneCursor& c) {
  const int64_t n = b->cfg.n_lanes;
  hipStream_t st = b->ctx->stream;
  if (b->gen_env)
    HIP_TRY(launch_generic_cursor(b->bk_lmem.p, n, c, st));
  else if (b->fc16_env)
    HIP_TRY(launch_fc16_cursor(b->bk_slots.p, n, c, st));
  else if (b->is_eth)
    HIP_TRY(launch_eth_cursor(b->bk_slots.p, n, c, st));
  else if (b->cfg.protocol == CPR_PROTO_BK)
    HIP_TRY(launch_bk_cursor(b->bk_slots.p, n, c, st));
  else if (b->cfg.protocol == CPR_PROTO_TAILSTORM)
    HIP_TRY(launch_ts_cursor(b->bk_slots.p, n, c, st));
  else
    HIP_TRY(launch_lock_cursor(lock_buffers(b), n, c, st));
  return CPR_OK;
}

// ---------------------------------------------------------------- lane env (cpr-v0 layers)

int cpr_lane_env_set(cpr_batch* b, const cpr_lane_env* env) {
  if (!b || !env) return fail(CPR_E_INVALID_ARG, "NULL argument");
  CPR_ENTER(b->ctx);
  if (b->cfg.protocol == CPR_PROTO_FC16)
    return fail(CPR_E_UNSUPPORTED, "FC16 runs fused episodes (cpr_run_episodes) only");
  if (b->cfg.n_lanes <= 0 || b->cfg.mode != CPR_MODE_GYM)
    return fail(CPR_E_UNSUPPORTED, "a lane env needs lockstep lanes (CPR_MODE_GYM, "
                                   "cfg.n_lanes > 0)");
  if (b->reset_done)
    return fail(CPR_E_STATE, "cpr_lane_env_set after the batch's first reset or rollout");
  const bool table = env->n_alpha != 0 || env->alpha != nullptr;
  if (table && (env->n_alpha < 1 || env->n_alpha > kLaneEnvMaxAlpha || !env->alpha))
    return fail(CPR_E_INVALID_ARG, "lane env: n_alpha must be in 1..4096 with a table (or 0 and "
                                   "NULL for cfg.alpha)");
  if (env->gym_reward < CPR_GYM_REWARD_ENGINE || env->gym_reward > CPR_GYM_REWARD_DENSE_PER_PROGRESS)
    return fail(CPR_E_INVALID_ARG, "lane env: unknown gym_reward");
  if (env->reward_shape < CPR_SHAPE_NONE || env->reward_shape > CPR_SHAPE_CUT)
    return fail(CPR_E_INVALID_ARG, "lane env: unknown reward_shape");
  if (env->gym_reward == CPR_GYM_REWARD_DENSE_PER_PROGRESS && b->fc16_env)
    return fail(CPR_E_UNSUPPORTED, "lane env: the FC16 model has no progress target "
                                   "(CPR_GYM_REWARD_DENSE_PER_PROGRESS)");
  if (env->gym_reward == CPR_GYM_REWARD_DENSE_PER_PROGRESS && b->gen_env)
    return fail(CPR_E_UNSUPPORTED, "lane env: the generic env has no progress target "
                                   "(CPR_GYM_REWARD_DENSE_PER_PROGRESS)");
  if (env->gym_reward == CPR_GYM_REWARD_DENSE_PER_PROGRESS && !(env->dense_target > 0.0))
    return fail(CPR_E_INVALID_ARG, "lane env: dense_target <= 0");
  if (env->alpha_column < -1)
    return fail(CPR_E_INVALID_ARG, "lane env: alpha_column < -1");
  if (b->has_net && env->alpha_column >= b->pn.n_extra)
    return fail(CPR_E_INVALID_ARG, "lane env: alpha_column >= n_extra of the batch's network");
  std::vector<double> tab_a(table ? env->alpha : &b->cfg.alpha,
                            table ? env->alpha + env->n_alpha : &b->cfg.alpha + 1);
  const bool divides = env->reward_shape != CPR_SHAPE_NONE;
  for (double a : tab_a) {
    if (std::isnan(a)) return fail(CPR_E_INVALID_ARG, "alpha cannot be NaN");
    if (a < 0. || a > 1.) return fail(CPR_E_INVALID_ARG, "alpha < 0 || alpha > 1");
    if (divides && !(a > 0.))
      return fail(CPR_E_INVALID_ARG, "lane env: the reward shape divides by alpha, which is 0");
  }
  std::vector<uint64_t> tab_t(tab_a.size());
  for (size_t i = 0; i < tab_a.size(); i++) tab_t[i] = alpha_threshold(tab_a[i]);
  HIP_TRY(hipSetDevice(b->ctx->device));
  const size_t n = (size_t)b->cfg.n_lanes;
  // before the first reset every lane stands at cfg.alpha
  const std::vector<double> la(n, b->cfg.alpha), zero(n, 0.0);
  const std::vector<uint64_t> lt(n, alpha_threshold(b->cfg.alpha));
  HIP_TRY(b->le_tab_t.ensure(tab_t.size() * 8));
  HIP_TRY(b->le_tab_a.ensure(tab_a.size() * 8));
  HIP_TRY(b->le_lane_t.ensure(n * 8));
  HIP_TRY(b->le_lane_a.ensure(n * 8));
  HIP_TRY(b->le_acc.ensure(n * 8));
  HIP_TRY(hipMemcpy(b->le_tab_t.p, tab_t.data(), tab_t.size() * 8, hipMemcpyHostToDevice));
  HIP_TRY(hipMemcpy(b->le_tab_a.p, tab_a.data(), tab_a.size() * 8, hipMemcpyHostToDevice));
  HIP_TRY(hipMemcpy(b->le_lane_t.p, lt.data(), n * 8, hipMemcpyHostToDevice));
  HIP_TRY(hipMemcpy(b->le_lane_a.p, la.data(), n * 8, hipMemcpyHostToDevice));
  HIP_TRY(hipMemcpy(b->le_acc.p, zero.data(), n * 8, hipMemcpyHostToDevice));
  b->env = *env;
  b->env.alpha = nullptr;
  b->env.n_alpha = (int32_t)tab_a.size();
  b->env_table = table;
  b->has_env = true;
  return CPR_OK;
}

int cpr_lane_alpha(cpr_batch* b, double* alpha) {
  if (!b || !alpha) return fail(CPR_E_INVALID_ARG, "NULL argument");
  CPR_ENTER(b->ctx);
  const int64_t n = b->cfg.n_lanes;
  if (!b->has_env) {
    for (int64_t i = 0; i < n; i++) alpha[i] = b->cfg.alpha;
    return CPR_OK;
  }
  HIP_TRY(hipSetDevice(b->ctx->device));
  hipStream_t st = b->ctx->stream;
  HIP_TRY(hipMemcpyAsync(alpha, b->le_lane_a.p, (size_t)n * 8, hipMemcpyDeviceToHost, st));
  HIP_TRY(hipStreamSynchronize(st));
  return CPR_OK;
}

int cpr_rollout_net(cpr_batch* b, int64_t n_steps, int deterministic,
                    const cpr_rollout_net_out* out, int outputs_on_device,
                    cpr_summary* summary) {
  return cpr_rollout_net_env(b, n_steps, deterministic, out, nullptr, outputs_on_device, summary);
}

// slot `slot` of the replay ring
static DqnRows dqn_slot(const cpr_batch* b, int64_t slot) {
  const size_t r = (size_t)slot * (size_t)b->cfg.n_lanes, ol = (size_t)b->pn.obs_len;
  DqnRows S;
  S.obs = (float*)b->dq_obs.p + r * ol;
  S.next_obs = (float*)b->dq_next.p + r * ol;
  S.alpha = (double*)b->dq_alpha.p + r;
  S.action = (int32_t*)b->dq_action.p + r;
  S.reward = (double*)b->dq_reward.p + r;
  S.done = (uint8_t*)b->dq_done.p + r;
  return S;
}

static int rollout_net_run(cpr_batch* b, int64_t n_steps, int deterministic,
                           const cpr_rollout_net_out* out, const cpr_rollout_env_out* env_out,
                           int outputs_on_device, cpr_summary* summary, const double* dqn_epsilon);

int cpr_rollout_net_env(cpr_batch* b, int64_t n_steps, int deterministic,
                        const cpr_rollout_net_out* out, const cpr_rollout_env_out* env_out,
                        int outputs_on_device, cpr_summary* summary) {
  return rollout_net_run(b, n_steps, deterministic, out, env_out, outputs_on_device, summary,
                         nullptr);
}

// cpr_rollout_net_env, and with dqn_epsilon cpr_dqn_collect: the same launch sequence with the
// epsilon-greedy forward (k_dqn_act) in k_policy_forward's place, no step-major outputs, and
// step t's transitions written to slot (cursor + t) mod capacity of the replay ring
static int rollout_net_run(cpr_batch* b, int64_t n_steps, int deterministic,
                           const cpr_rollout_net_out* out, const cpr_rollout_env_out* env_out,
                           int outputs_on_device, cpr_summary* summary, const double* dqn_epsilon) {
  if (!b || !summary) return fail(CPR_E_INVALID_ARG, "NULL argument");
  CPR_ENTER(b->ctx);
  if (b->cfg.protocol == CPR_PROTO_FC16)
    return fail(CPR_E_UNSUPPORTED, "FC16 runs fused episodes (cpr_run_episodes) only");
  if (!b->has_net) return fail(CPR_E_STATE, "no policy network set (cpr_policy_net_set)");
  if (b->parked) return fail(CPR_E_STATE, "rollout after cpr_eval_net without a reset");
  if (b->gen_env) {
    const char* fq = getenv("CPR_FC16_ROLLOUT_FUSED");
    if (fq && fq[0] != '0')
      return fail(CPR_E_UNSUPPORTED, "CPR_FC16_ROLLOUT_FUSED: the one-kernel rollout holds an "
                                     "FC16 slot in registers; the generic env's block DAG does "
                                     "not fit there");
  }
  if (n_steps <= 0) return CPR_OK;
  HIP_TRY(hipSetDevice(b->ctx->device));
  int rc = ensure_lockstep(b);
  if (rc) return rc;
  const int64_t n = b->cfg.n_lanes;
  const int ol = obs_len_of(b->cfg);
  const int64_t cells = n_steps * n;
  hipStream_t st = b->ctx->stream;
  HIP_TRY(b->summary.ensure(sizeof(cpr_summary)));
  HIP_TRY(hipMemsetAsync(b->summary.p, 0, sizeof(cpr_summary), st));
  if (!b->ev0) {
    HIP_TRY(hipEventCreate(&b->ev0));
    HIP_TRY(hipEventCreate(&b->ev1));
  }
  HIP_TRY(b->pn_step.ensure((size_t)n * 8));
  HIP_TRY(b->pn_acts0.ensure((size_t)n * 8));
  HIP_TRY(b->pn_acts.ensure((size_t)n * 8));
  // outputs: the caller's device buffers, or library-owned staging copied back at the end
  cpr_rollout_net_out H = {};
  if (out) H = *out;
  cpr_rollout_net_out D = H;
  cpr_rollout_env_out HE = {};
  if (env_out) HE = *env_out;
  cpr_rollout_env_out DE = HE;
  struct Stage {
    void** dev;
    void* host;
    size_t bytes;
    DevBuf buf;
  };
  Stage stage[10] = {{(void**)&D.obs0, H.obs0, (size_t)n * ol * 8, {}},
                    {(void**)&D.obs, H.obs, (size_t)cells * ol * 8, {}},
                    {(void**)&D.action, H.action, (size_t)cells * 4, {}},
                    {(void**)&D.reward, H.reward, (size_t)cells * 8, {}},
                    {(void**)&D.done, H.done, (size_t)cells, {}},
                    {(void**)&D.logp, H.logp, (size_t)cells * 8, {}},
                    {(void**)&D.value, H.value, (size_t)(cells + n) * 8, {}},
                    {(void**)&DE.alpha0, HE.alpha0, (size_t)n * 8, {}},
                    {(void**)&DE.alpha, HE.alpha, (size_t)cells * 8, {}},
                    {(void**)&DE.engine_reward, HE.engine_reward, (size_t)cells * 8, {}}};
  if (!outputs_on_device)
    for (Stage& s : stage)
      if (s.host) {
        HIP_TRY(s.buf.ensure(s.bytes));
        *s.dev = s.buf.p;
      }
  const StepBuffers sb = step_buffers(b);
  HIP_TRY(hipEventRecord(b->ev0, st));
  // a first call without a reset starts lane i at episode i (that reset's activations count,
  // as in the built-in rollout); otherwise the reset kernel with an empty mask resets nothing
  // and writes every lane's current observation into l_obs (cpr_rollout leaves none there)
  const bool fresh = !b->reset_done;
  if (!fresh) HIP_TRY(hipMemsetAsync(b->l_mask.p, 0, (size_t)n, st));
  // without a lane env every episode runs at cfg.alpha: the alpha outputs are that constant
  const bool env = b->has_env;
  if (!env && (DE.alpha0 || DE.alpha)) {
    const std::vector<double> ca((size_t)(DE.alpha ? cells : n), b->cfg.alpha);
    if (DE.alpha0) HIP_TRY(hipMemcpyAsync(DE.alpha0, ca.data(), (size_t)n * 8, hipMemcpyHostToDevice, st));
    if (DE.alpha) HIP_TRY(hipMemcpyAsync(DE.alpha, ca.data(), (size_t)cells * 8, hipMemcpyHostToDevice, st));
    HIP_TRY(hipStreamSynchronize(st));  // ca leaves scope
  }
  rc = launch_lock_reset(b, fresh ? nullptr : (const uint8_t*)b->l_mask.p, nullptr, sb.obs,
                         env ? DE.alpha0 : nullptr);
  if (rc) return rc;
  LaneCursor cur;
  cur.ep = (uint64_t*)b->l_eps.p;
  cur.steps = (int64_t*)b->pn_step.p;
  cur.acts = (int64_t*)b->pn_acts0.p;
  rc = launch_lane_cursor(b, cur);
  if (rc) return rc;
  if (fresh) HIP_TRY(hipMemsetAsync(b->pn_acts0.p, 0, (size_t)n * 8, st));
  if (D.obs0)
    HIP_TRY(hipMemcpyAsync(D.obs0, sb.obs, (size_t)n * ol * 8, hipMemcpyDeviceToDevice, st));
  PolIO io = {};
  io.n = n;
  io.deterministic = deterministic ? 1 : 0;
  io.seed = b->cfg.seed;
  io.ep = cur.ep;
  io.step = cur.steps;
  io.alpha_col = -1;
  if (env && b->env.alpha_column >= 0) {
    io.lane_alpha = (const double*)b->le_lane_a.p;
    io.alpha_col = b->env.alpha_column;
  }
  PolCollect C = {};
  C.reward = sb.reward;
  C.done = sb.done;
  C.era = sb.era;
  C.erd = sb.erd;
  C.eprog = sb.eprog;
  C.esteps = sb.esteps;
  C.eacts = sb.eacts;
  C.hh = sb.hh;
  C.status = sb.status;
  C.orphans_from_progress = b->is_ev ? 1 : 0;
  C.ep = cur.ep;
  C.step = cur.steps;
  C.acts0 = cur.acts;
  C.mask = (uint8_t*)b->l_mask.p;
  C.sum = (cpr_summary*)b->summary.p;
  if (env) {
    C.gym_reward = b->env.gym_reward;
    C.reward_shape = b->env.reward_shape;
    C.dense_target = b->env.dense_target;
    C.lane_alpha = (const double*)b->le_lane_a.p;
    C.dense_acc = (double*)b->le_acc.p;
  }
  // FC16 env lanes with CPR_FC16_ROLLOUT_FUSED=1 (read at every call): every step, the
  // bootstrap row and the tail in one kernel, unless its LDS does not fit
  // the device. Off by default: it computes the same bits as the launch sequence below and is
  // faster at 4,096 lanes, but loses to it at 65,536 lanes x 3 x 64
  // (profiles/fc16_rollout_speed.json); CPR_FC16_ROLLOUT_FUSED=0 names the default
#ifndef CPR_FC16_ROLLOUT_FUSED_DEFAULT
#define CPR_FC16_ROLLOUT_FUSED_DEFAULT 0
#endif
  const char* fv = getenv("CPR_FC16_ROLLOUT_FUSED");
  const bool want_fused = fv ? fv[0] != '0' : CPR_FC16_ROLLOUT_FUSED_DEFAULT != 0;
  const bool fused = !dqn_epsilon && b->fc16_env && want_fused && fc16_rollout_net_fits(b->pn);
  b->roll_fused = fused;
  if (fused) {
    Fc16Roll R = {};
    R.P = b->FP;
    R.seed = b->cfg.seed;
    R.slots = b->bk_slots.p;
    R.n = n;
    R.n_steps = n_steps;
    R.deterministic = deterministic ? 1 : 0;
    R.fresh = fresh ? 1 : 0;
    R.obs = D.obs;
    R.action = D.action;
    R.reward = D.reward;
    R.done = D.done;
    R.logp = D.logp;
    R.value = D.value;
    R.alpha = env ? DE.alpha : nullptr;
    R.engine_reward = DE.engine_reward;
    R.sum = (cpr_summary*)b->summary.p;
    R.alpha_col = -1;
    if (env) {
      R.n_alpha = b->env.n_alpha;
      R.schedule = b->schedule;
      R.gym_reward = b->env.gym_reward;
      R.reward_shape = b->env.reward_shape;
      R.alpha_col = b->env.alpha_column;
      R.dense_target = b->env.dense_target;
      R.tab_t = (const uint64_t*)b->le_tab_t.p;
      R.tab_a = (const double*)b->le_tab_a.p;
      R.lane_t = (uint64_t*)b->le_lane_t.p;
      R.lane_alpha = (double*)b->le_lane_a.p;
      R.dense_acc = (double*)b->le_acc.p;
    }
    HIP_TRY(launch_fc16_rollout_net(b->pn, R, st));
  }
  // the policy input of step t: l_obs before the first step, then where the reset kernel
  // of step t - 1 wrote every lane's observation (the caller's obs row, or l_obs)
  const double* in_obs = sb.obs;
  for (int64_t t = 0; t < n_steps && !fused; ++t) {
    int32_t* act = D.action ? D.action + t * n : (int32_t*)b->l_act.p;
    DqnRows slot = {};
    if (dqn_epsilon) {
      slot = dqn_slot(b, (b->dq_cursor + t) % b->dq_cap);
      DqnAct A = {};
      A.obs = in_obs;
      A.n = n;
      A.epsilon = *dqn_epsilon;
      A.seed = b->cfg.seed;
      A.ep = cur.ep;
      A.step = cur.steps;
      A.lane_alpha = env ? (const double*)b->le_lane_a.p : nullptr;
      A.alpha_col = io.alpha_col;
      A.cfg_alpha = b->cfg.alpha;
      A.action = act;
      A.slot = slot;
      HIP_TRY(launch_dqn_act(b->pn, A, st));
    } else {
      io.obs = in_obs;
      io.action = act;
      io.logp = D.logp ? D.logp + t * n : nullptr;
      io.value = D.value ? D.value + t * n : nullptr;
      HIP_TRY(launch_policy_forward(b->pn, io, st));
    }
    rc = launch_lock_step(b, act, sb, true);
    if (rc) return rc;
    C.out_reward = dqn_epsilon ? slot.reward : D.reward ? D.reward + t * n : nullptr;
    C.out_done = dqn_epsilon ? slot.done : D.done ? D.done + t * n : nullptr;
    C.out_engine_reward = DE.engine_reward ? DE.engine_reward + t * n : nullptr;
    HIP_TRY(launch_policy_collect(C, n, st));
    double* next_obs = D.obs ? D.obs + t * n * ol : sb.obs;
    rc = launch_lock_reset(b, C.mask, cur.ep, next_obs,
                           env && DE.alpha ? DE.alpha + t * n : nullptr);
    if (rc) return rc;
    if (dqn_epsilon) HIP_TRY(launch_dqn_store(next_obs, n * ol, slot.next_obs, st));
    in_obs = next_obs;
  }
  if (D.value && !fused) {  // PPO's bootstrap: the value of the final observation
    io.obs = in_obs;
    io.deterministic = 1;
    io.action = nullptr;
    io.logp = nullptr;
    io.value = D.value + cells;
    HIP_TRY(launch_policy_forward(b->pn, io, st));
  }
  if (!fused) {  // activations of the episodes still running
    LaneCursor end = cur;
    end.acts = (int64_t*)b->pn_acts.p;
    rc = launch_lane_cursor(b, end);
    if (rc) return rc;
    HIP_TRY(launch_policy_tail(end.acts, cur.acts, n, C.sum, st));
  }
  HIP_TRY(hipEventRecord(b->ev1, st));
  cpr_summary s;
  HIP_TRY(hipMemcpyAsync(&s, b->summary.p, sizeof(s), hipMemcpyDeviceToHost, st));
  if (!outputs_on_device)
    for (Stage& g : stage)
      if (g.host) HIP_TRY(hipMemcpyAsync(g.host, *g.dev, g.bytes, hipMemcpyDeviceToHost, st));
  HIP_TRY(hipStreamSynchronize(st));
  float ms = 0.f;
  HIP_TRY(hipEventElapsedTime(&ms, b->ev0, b->ev1));
  b->last_ms = ms;
  b->last_acts = s.activations;
  b->async_launch = false;
  b->reset_done = true;
  b->last_lanes = n;
  b->last_resident = n;
  if (dqn_epsilon) {
    b->dq_cursor = (b->dq_cursor + n_steps) % b->dq_cap;
    b->dq_size = std::min(b->dq_cap, b->dq_size + n_steps);
    b->dq_steps += n_steps;
  }
  summary->episodes += s.episodes;
  summary->steps += s.steps;
  summary->activations += s.activations;
  summary->reward_attacker_fx += s.reward_attacker_fx;
  summary->reward_defender_fx += s.reward_defender_fx;
  summary->progress_fx += s.progress_fx;
  summary->rel_revenue_fx += s.rel_revenue_fx;
  summary->rel_revenue_sq_fx += s.rel_revenue_sq_fx;
  summary->orphans += s.orphans;
  summary->status_tie += s.status_tie;
  summary->status_overlap += s.status_overlap;
  summary->status_other += s.status_other;
  summary->invalid += s.invalid;
  for (int i = 0; i < CPR_HIST_BINS; i++) summary->hist[i] += s.hist[i];
  return CPR_OK;
}

int cpr_rollout_net_fused(cpr_batch* b, int32_t* fused) {
  if (!b || !fused) return fail(CPR_E_INVALID_ARG, "NULL argument");
  CPR_ENTER(b->ctx);
  *fused = b->roll_fused ? 1 : 0;
  return CPR_OK;
}

int cpr_lane_env_schedule(cpr_batch* b, int schedule) {
  if (!b) return fail(CPR_E_INVALID_ARG, "NULL argument");
  CPR_ENTER(b->ctx);
  if (b->cfg.protocol == CPR_PROTO_FC16)
    return fail(CPR_E_UNSUPPORTED, "FC16 runs fused episodes (cpr_run_episodes) only");
  if (b->cfg.n_lanes <= 0 || b->cfg.mode != CPR_MODE_GYM)
    return fail(CPR_E_UNSUPPORTED, "a lane env needs lockstep lanes (CPR_MODE_GYM, "
                                   "cfg.n_lanes > 0)");
  if (b->reset_done)
    return fail(CPR_E_STATE, "cpr_lane_env_schedule after the batch's first reset or rollout");
  if (schedule != CPR_SCHEDULE_CHOICE && schedule != CPR_SCHEDULE_CYCLE)
    return fail(CPR_E_INVALID_ARG, "lane env: unknown schedule");
  b->schedule = schedule;
  return CPR_OK;
}

// ---------------------------------------------------------------- evaluation (cpr_eval_net)

static void summary_add(cpr_summary* d, const cpr_summary& s) {
  d->episodes += s.episodes;
  d->steps += s.steps;
  d->activations += s.activations;
  d->reward_attacker_fx += s.reward_attacker_fx;
  d->reward_defender_fx += s.reward_defender_fx;
  d->progress_fx += s.progress_fx;
  d->rel_revenue_fx += s.rel_revenue_fx;
  d->rel_revenue_sq_fx += s.rel_revenue_sq_fx;
  d->orphans += s.orphans;
  d->status_tie += s.status_tie;
  d->status_overlap += s.status_overlap;
  d->status_other += s.status_other;
  d->invalid += s.invalid;
  for (int i = 0; i < CPR_HIST_BINS; i++) d->hist[i] += s.hist[i];
}

int cpr_eval_net(cpr_batch* b, const cpr_eval_opts* opts, cpr_eval_record* records,
                 cpr_eval_alpha* per_alpha, cpr_summary* per_alpha_summary, cpr_summary* total) {
  if (!b || !opts || !per_alpha) return fail(CPR_E_INVALID_ARG, "NULL argument");
  CPR_ENTER(b->ctx);
  if (b->cfg.protocol == CPR_PROTO_FC16)
    return fail(CPR_E_UNSUPPORTED, "FC16 runs fused episodes (cpr_run_episodes) only");
  if (!b->has_net) return fail(CPR_E_STATE, "no policy network set (cpr_policy_net_set)");
  if (opts->episodes_per_alpha < 1)
    return fail(CPR_E_INVALID_ARG, "eval: episodes_per_alpha must be >= 1");
  if (opts->check_every < 0) return fail(CPR_E_INVALID_ARG, "eval: check_every < 0");
  const int64_t max_steps = b->cfg.max_steps;
  if (max_steps <= 0)
    return fail(CPR_E_UNSUPPORTED, "eval: cfg.max_steps <= 0 leaves an episode's length unbounded");
  const bool env = b->has_env;
  const int32_t A = env ? b->env.n_alpha : 1;
  if (A > 1 && b->schedule != CPR_SCHEDULE_CYCLE)
    return fail(CPR_E_UNSUPPORTED, "eval: a table of several alphas needs CPR_SCHEDULE_CYCLE "
                                   "(cpr_lane_env_schedule): a keyed choice gives its alphas "
                                   "unequal shares of the set");
  if (opts->episodes_per_alpha > (int64_t)((1ull << 40) / (uint64_t)A))
    return fail(CPR_E_INVALID_ARG, "eval: more than 2^40 episodes");
  const int64_t epa = opts->episodes_per_alpha, n_set = epa * A;
  HIP_TRY(hipSetDevice(b->ctx->device));
  int rc = ensure_lockstep(b);
  if (rc) return rc;
  const int64_t n = b->cfg.n_lanes;
  hipStream_t st = b->ctx->stream;
  if (!b->ev0) {
    HIP_TRY(hipEventCreate(&b->ev0));
    HIP_TRY(hipEventCreate(&b->ev1));
  }
  HIP_TRY(b->pn_step.ensure((size_t)n * 8));
  HIP_TRY(b->ev_rec.ensure((size_t)n_set * sizeof(cpr_eval_record)));
  HIP_TRY(b->ev_acc.ensure((size_t)n * 8));
  HIP_TRY(b->ev_cnt.ensure(8));
  HIP_TRY(b->ev_sum.ensure((size_t)A * sizeof(cpr_summary)));
  HIP_TRY(b->ev_alpha.ensure((size_t)A * sizeof(cpr_eval_alpha)));
  {  // SB3's evaluate_policy begins with a reset: lane i to episode first_episode + i
    std::vector<uint64_t> ids((size_t)n);
    for (int64_t i = 0; i < n; i++) ids[(size_t)i] = opts->first_episode + (uint64_t)i;
    HIP_TRY(hipMemcpy(b->l_eps.p, ids.data(), (size_t)n * 8, hipMemcpyHostToDevice));
  }
  HIP_TRY(hipMemsetAsync(b->pn_step.p, 0, (size_t)n * 8, st));
  HIP_TRY(hipMemsetAsync(b->ev_rec.p, 0, (size_t)n_set * sizeof(cpr_eval_record), st));
  HIP_TRY(hipMemsetAsync(b->ev_acc.p, 0, (size_t)n * 8, st));
  HIP_TRY(hipMemsetAsync(b->ev_cnt.p, 0, 8, st));
  HIP_TRY(hipMemsetAsync(b->ev_sum.p, 0, (size_t)A * sizeof(cpr_summary), st));
  const StepBuffers sb = step_buffers(b);
  HIP_TRY(hipEventRecord(b->ev0, st));
  // from here on the lanes no longer stand where the caller left them
  b->reset_done = true;
  b->parked = true;
  uint64_t* ep = (uint64_t*)b->l_eps.p;
  rc = launch_lock_reset(b, nullptr, ep, sb.obs);
  if (rc) return rc;
  PolIO io = {};
  io.n = n;
  io.deterministic = opts->deterministic ? 1 : 0;
  io.seed = b->cfg.seed;
  io.ep = ep;
  io.step = (const int64_t*)b->pn_step.p;
  io.obs = sb.obs;
  io.action = (int32_t*)b->l_act.p;
  io.alpha_col = -1;
  if (env && b->env.alpha_column >= 0) {
    io.lane_alpha = (const double*)b->le_lane_a.p;
    io.alpha_col = b->env.alpha_column;
  }
  EvalCollect C = {};
  C.reward = sb.reward;
  C.done = sb.done;
  C.era = sb.era;
  C.erd = sb.erd;
  C.eprog = sb.eprog;
  C.ect = sb.ect;
  C.est = sb.est;
  C.esteps = sb.esteps;
  C.eacts = sb.eacts;
  C.hh = sb.hh;
  C.status = sb.status;
  C.orphans_from_progress = b->is_ev ? 1 : 0;
  C.ep = ep;
  C.step = (int64_t*)b->pn_step.p;
  C.mask = (uint8_t*)b->l_mask.p;
  C.ep_reward = (double*)b->ev_acc.p;
  C.cfg_alpha = b->cfg.alpha;
  C.n_alpha = A;
  C.schedule = b->schedule;
  C.seed = b->cfg.seed;
  if (env) {
    C.gym_reward = b->env.gym_reward;
    C.reward_shape = b->env.reward_shape;
    C.dense_target = b->env.dense_target;
    C.lane_alpha = (const double*)b->le_lane_a.p;
    C.dense_acc = (double*)b->le_acc.p;
  }
  C.first = opts->first_episode;
  C.n_set = n_set;
  C.records = (cpr_eval_record*)b->ev_rec.p;
  C.finished = (unsigned long long*)b->ev_cnt.p;
  // every episode ends within max_steps steps and a lane runs at most ceil(n_set / n) episodes
  // of the set, back to back from the first step: `bound` steps finish the set
  const int64_t rounds = (n_set + n - 1) / n;
  if (rounds > INT64_MAX / max_steps) return fail(CPR_E_INVALID_ARG, "eval: step bound overflows");
  const int64_t bound = rounds * max_steps;
  const int64_t every = opts->check_every > 0 ? opts->check_every : max_steps;
  int64_t t = 0;
  for (;;) {
    const int64_t chunk = std::min<int64_t>(every, bound - t);
    for (int64_t k = 0; k < chunk; ++k) {
      HIP_TRY(launch_policy_forward(b->pn, io, st));
      rc = launch_lock_step(b, io.action, sb, true);
      if (rc) return rc;
      HIP_TRY(launch_eval_collect(C, n, st));
      // a finished lane is reset before it is stepped again (its buffers are sized by max_steps)
      rc = launch_lock_reset(b, C.mask, ep, sb.obs);
      if (rc) return rc;
    }
    t += chunk;
    unsigned long long fin = 0;
    HIP_TRY(hipMemcpyAsync(&fin, C.finished, 8, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    if ((int64_t)fin == n_set) break;
    if (t >= bound)
      return fail(CPR_E_INTERNAL, "eval: " + std::to_string(fin) + " of " + std::to_string(n_set) +
                                      " episodes finished after " + std::to_string(bound) +
                                      " steps");
  }
  EvalReduce R = {};
  R.records = C.records;
  R.first = opts->first_episode;
  R.per_alpha = epa;
  R.n_alpha = A;
  R.tab_a = env ? (const double*)b->le_tab_a.p : nullptr;
  R.cfg_alpha = b->cfg.alpha;
  R.sums = (cpr_summary*)b->ev_sum.p;
  R.out = (cpr_eval_alpha*)b->ev_alpha.p;
  HIP_TRY(launch_eval_reduce(R, st));
  HIP_TRY(hipEventRecord(b->ev1, st));
  std::vector<cpr_summary> sums((size_t)A);
  HIP_TRY(hipMemcpyAsync(sums.data(), R.sums, (size_t)A * sizeof(cpr_summary),
                         hipMemcpyDeviceToHost, st));
  HIP_TRY(hipMemcpyAsync(per_alpha, R.out, (size_t)A * sizeof(cpr_eval_alpha),
                         hipMemcpyDeviceToHost, st));
  if (records)
    HIP_TRY(hipMemcpyAsync(records, C.records, (size_t)n_set * sizeof(cpr_eval_record),
                           hipMemcpyDeviceToHost, st));
  HIP_TRY(hipStreamSynchronize(st));
  cpr_summary tot = {};
  for (int32_t j = 0; j < A; j++) {
    if (per_alpha_summary) per_alpha_summary[j] = sums[(size_t)j];
    summary_add(&tot, sums[(size_t)j]);
  }
  if (total) *total = tot;
  float ms = 0.f;
  HIP_TRY(hipEventElapsedTime(&ms, b->ev0, b->ev1));
  b->last_ms = ms;
  b->last_acts = tot.activations;
  b->async_launch = false;
  b->last_lanes = n;
  b->last_resident = n;
  return CPR_OK;
}

int cpr_policy_net_copy(cpr_batch* dst, cpr_batch* src) {
  if (!dst || !src) return fail(CPR_E_INVALID_ARG, "NULL argument");
  CPR_ENTER(dst->ctx);
  if (dst->ctx != src->ctx)
    return fail(CPR_E_INVALID_ARG, "policy net copy: the batches belong to different contexts");
  if (!src->has_net) return fail(CPR_E_STATE, "policy net copy: the source has no network");
  if (dst == src) return CPR_OK;
  if (dst->cfg.protocol == CPR_PROTO_FC16)
    return fail(CPR_E_UNSUPPORTED, "FC16 runs fused episodes (cpr_run_episodes) only");
  if (dst->cfg.n_lanes <= 0 || dst->cfg.mode != CPR_MODE_GYM)
    return fail(CPR_E_UNSUPPORTED, "a policy network needs lockstep lanes (CPR_MODE_GYM, "
                                   "cfg.n_lanes > 0)");
  const PolNet& S = src->pn;
  int32_t ol = 0, na = 0;
  int rc = cpr_observation_spec(dst, &ol, &na, nullptr, nullptr);
  if (rc) return rc;
  if (ol != S.obs_len || na != S.n_actions)
    return fail(CPR_E_INVALID_ARG, "policy net copy: observation or action width differs");
  if (dst->has_net) {
    const PolNet& D = dst->pn;
    bool same = D.depth == S.depth && D.width_pi == S.width_pi && D.width_vf == S.width_vf &&
                D.n_extra == S.n_extra;
    for (int i = 0; same && i < S.n_extra; i++) same = D.extra[i] == S.extra[i];
    if (!same)
      return fail(CPR_E_INVALID_ARG, "policy net copy: depth, widths, n_extra or extras differ");
  }
  if (dst->has_env && dst->env.alpha_column >= S.n_extra)
    return fail(CPR_E_INVALID_ARG, "policy net: n_extra does not reach the lane env's "
                                   "alpha_column (cpr_lane_env_set)");
  HIP_TRY(hipSetDevice(dst->ctx->device));
  const int64_t lds = policy_lds_bytes(S.depth, S.width_pi, S.width_vf);
  if (lds > policy_lds_limit())
    return fail(CPR_E_UNSUPPORTED, "policy net: needs " + std::to_string(lds) +
                                       " B of LDS per workgroup, the device has " +
                                       std::to_string(policy_lds_limit()));
  hipStream_t st = dst->ctx->stream;
  const size_t bytes = (size_t)src->pn_total * sizeof(float);
  if (bytes > dst->pn_w.bytes) {
    // growing frees the old buffer: a forward of the previous network may still be reading it
    HIP_TRY(hipStreamSynchronize(st));
    HIP_TRY(dst->pn_w.ensure(bytes));
  }
  // stream ordered: behind the source's updates, before the destination's next forward
  HIP_TRY(hipMemcpyAsync(dst->pn_w.p, src->pn_w.p, bytes, hipMemcpyDeviceToDevice, st));
  PolNet N = S;
  const float* sbase = (const float*)src->pn_w.p;
  const float* dbase = (const float*)dst->pn_w.p;
  for (PolLayer* Ls : {N.pi, N.vf})
    for (int l = 0; l <= N.depth; l++) {
      Ls[l].W = dbase + (Ls[l].W - sbase);
      Ls[l].b = dbase + (Ls[l].b - sbase);
    }
  dst->pn_off = src->pn_off;
  dst->pn_cnt = src->pn_cnt;
  dst->pn_total = src->pn_total;
  dst->ppo_t = 0;
  dst->ppo_updates = 0;
  if (dst->pp_m.p) HIP_TRY(hipMemsetAsync(dst->pp_m.p, 0, dst->pp_m.bytes, st));
  if (dst->pp_v.p) HIP_TRY(hipMemsetAsync(dst->pp_v.p, 0, dst->pp_v.bytes, st));
  if (!dst->has_net) dst->pp_part.release();
  dst->pn = N;
  dst->has_net = true;
  if (dst->dq_ready) return dqn_target_reset(dst);
  return CPR_OK;
}

// ---------------------------------------------------------------- the learner (ppo.h)

int cpr_gae(cpr_batch* b, int64_t n_steps, const double* reward, const uint8_t* done,
            const double* value, double gamma, double lam, double* adv_out, double* ret_out,
            int on_device) {
  if (!b || !reward || !done || !value || !adv_out || !ret_out)
    return fail(CPR_E_INVALID_ARG, "NULL argument");
  CPR_ENTER(b->ctx);
  const int64_t n = b->cfg.n_lanes;
  if (n <= 0) return fail(CPR_E_UNSUPPORTED, "gae needs lockstep lanes (cfg.n_lanes > 0)");
  if (n_steps < 1) return fail(CPR_E_INVALID_ARG, "gae: n_steps must be >= 1");
  if (!std::isfinite(gamma) || !std::isfinite(lam))
    return fail(CPR_E_INVALID_ARG, "gae: non-finite gamma or lambda");
  HIP_TRY(hipSetDevice(b->ctx->device));
  hipStream_t st = b->ctx->stream;
  const size_t cells = (size_t)(n_steps * n);
  if (on_device) {
    HIP_TRY(launch_gae(n_steps, n, reward, done, value, gamma, lam, adv_out, ret_out, st));
    HIP_TRY(hipStreamSynchronize(st));
    return CPR_OK;
  }
  DevBuf r, d, v, a, q;
  HIP_TRY(r.ensure(cells * 8));
  HIP_TRY(d.ensure(cells));
  HIP_TRY(v.ensure((cells + (size_t)n) * 8));
  HIP_TRY(a.ensure(cells * 8));
  HIP_TRY(q.ensure(cells * 8));
  HIP_TRY(hipMemcpyAsync(r.p, reward, cells * 8, hipMemcpyHostToDevice, st));
  HIP_TRY(hipMemcpyAsync(d.p, done, cells, hipMemcpyHostToDevice, st));
  HIP_TRY(hipMemcpyAsync(v.p, value, (cells + (size_t)n) * 8, hipMemcpyHostToDevice, st));
  HIP_TRY(launch_gae(n_steps, n, (const double*)r.p, (const uint8_t*)d.p, (const double*)v.p,
                     gamma, lam, (double*)a.p, (double*)q.p, st));
  HIP_TRY(hipMemcpyAsync(adv_out, a.p, cells * 8, hipMemcpyDeviceToHost, st));
  HIP_TRY(hipMemcpyAsync(ret_out, q.p, cells * 8, hipMemcpyDeviceToHost, st));
  HIP_TRY(hipStreamSynchronize(st));
  return CPR_OK;
}

int cpr_ppo_opts_default(cpr_ppo_opts* o) {
  if (!o) return fail(CPR_E_INVALID_ARG, "NULL argument");
  *o = cpr_ppo_opts{};
  o->n_epochs = 10;
  o->minibatch = 64;
  o->clip_range = 0.1;
  o->ent_coef = 0.0;
  o->vf_coef = 0.5;
  o->max_grad_norm = 0.5;
  o->lr = 3e-4;
  o->beta1 = 0.9;
  o->beta2 = 0.999;
  o->adam_eps = 1e-5;
  o->normalize_advantage = 1;
  o->gae_gamma = 0.99;
  o->gae_lambda = 0.95;
  o->perm_seed = 0;
  return CPR_OK;
}

// state, shapes and options of every cpr_ppo_* call, before anything is launched
static int ppo_check(cpr_batch* b, const cpr_ppo_opts* o) {
  if (!b || !o) return fail(CPR_E_INVALID_ARG, "NULL argument");
  if (b->cfg.protocol == CPR_PROTO_FC16)
    return fail(CPR_E_UNSUPPORTED, "FC16 runs fused episodes (cpr_run_episodes) only");
  if (!b->has_net) return fail(CPR_E_STATE, "no policy network set (cpr_policy_net_set)");
  if (o->n_epochs < 1) return fail(CPR_E_INVALID_ARG, "ppo: n_epochs must be >= 1");
  if (o->minibatch < 1) return fail(CPR_E_INVALID_ARG, "ppo: minibatch must be >= 1");
  if (o->minibatch > INT32_MAX) return fail(CPR_E_INVALID_ARG, "ppo: minibatch above 2^31 - 1");
  const struct {
    const char* name;
    double v;
    bool positive;
  } fields[] = {{"clip_range", o->clip_range, true},      {"ent_coef", o->ent_coef, false},
                {"vf_coef", o->vf_coef, false},           {"max_grad_norm", o->max_grad_norm, true},
                {"lr", o->lr, false},                     {"beta1", o->beta1, false},
                {"beta2", o->beta2, false},               {"adam_eps", o->adam_eps, false},
                {"gae_gamma", o->gae_gamma, false},       {"gae_lambda", o->gae_lambda, false}};
  for (const auto& f : fields) {
    if (!std::isfinite(f.v)) return fail(CPR_E_INVALID_ARG, std::string("ppo: non-finite ") + f.name);
    if (f.positive && !(f.v > 0.0))
      return fail(CPR_E_INVALID_ARG, std::string("ppo: ") + f.name + " must be > 0");
  }
  if (!(o->beta1 >= 0.0 && o->beta1 < 1.0) || !(o->beta2 >= 0.0 && o->beta2 < 1.0))
    return fail(CPR_E_INVALID_ARG, "ppo: beta1 and beta2 must be in [0, 1)");
  HIP_TRY(hipSetDevice(b->ctx->device));
  const int64_t lds = ppo_lds_bytes(b->pn.depth, b->pn.width_pi, b->pn.width_vf);
  if (lds > ppo_lds_limit())
    return fail(CPR_E_UNSUPPORTED,
                "ppo: the training forward of this network needs " + std::to_string(lds) +
                    " B of LDS per workgroup, the device has " + std::to_string(ppo_lds_limit()));
  return CPR_OK;
}

// the training data on the device: the caller's pointers, or staged copies
struct PpoDev {
  int64_t n;
  const double* obs;
  const double* alpha;  // null unless the lane env feeds an alpha column
  int32_t alpha_col;
  const int32_t* action;
  const double* old_logp;
  const double* adv;
  const double* ret;
};

static int ppo_stage(cpr_batch* b, const cpr_ppo_data* d, PpoDev* out) {
  if (!d) return fail(CPR_E_INVALID_ARG, "NULL argument");
  if (d->n < 1) return fail(CPR_E_INVALID_ARG, "ppo: data.n must be >= 1");
  if (d->n > INT32_MAX) return fail(CPR_E_INVALID_ARG, "ppo: data.n above 2^31 - 1 (int32 rows)");
  if (!d->obs || !d->action || !d->old_logp || !d->advantage || !d->ret)
    return fail(CPR_E_INVALID_ARG, "ppo: NULL data array");
  const bool use_alpha = b->has_env && b->env.alpha_column >= 0;
  if (use_alpha && !d->alpha)
    return fail(CPR_E_INVALID_ARG, "ppo: data.alpha is NULL but the lane env names an alpha column");
  PpoDev D = {};
  D.n = d->n;
  D.alpha_col = use_alpha ? b->env.alpha_column : -1;
  if (d->on_device) {
    D.obs = d->obs;
    D.alpha = use_alpha ? d->alpha : nullptr;
    D.action = d->action;
    D.old_logp = d->old_logp;
    D.adv = d->advantage;
    D.ret = d->ret;
    *out = D;
    return CPR_OK;
  }
  const size_t n = (size_t)d->n;
  const int na = b->pn.n_actions;
  for (size_t i = 0; i < n; i++)
    if (d->action[i] < 0 || d->action[i] >= na)
      return fail(CPR_E_INVALID_ARG, "ppo: data.action out of range");
  hipStream_t st = b->ctx->stream;
  struct {
    DevBuf* buf;
    const void* src;
    size_t bytes;
  } cp[] = {{&b->pp_obs, d->obs, n * (size_t)b->pn.obs_len * 8},
            {&b->pp_alpha, use_alpha ? d->alpha : nullptr, n * 8},
            {&b->pp_action, d->action, n * 4},
            {&b->pp_logp, d->old_logp, n * 8},
            {&b->pp_adv, d->advantage, n * 8},
            {&b->pp_ret, d->ret, n * 8}};
  for (auto& c : cp) {
    if (!c.src) continue;
    HIP_TRY(c.buf->ensure(c.bytes));
    HIP_TRY(hipMemcpyAsync(c.buf->p, c.src, c.bytes, hipMemcpyHostToDevice, st));
  }
  D.obs = (const double*)b->pp_obs.p;
  D.alpha = use_alpha ? (const double*)b->pp_alpha.p : nullptr;
  D.action = (const int32_t*)b->pp_action.p;
  D.old_logp = (const double*)b->pp_logp.p;
  D.adv = (const double*)b->pp_adv.p;
  D.ret = (const double*)b->pp_ret.p;
  *out = D;
  return CPR_OK;
}

// rows of the weight gradient's row blocks for a minibatch of B rows: at most
// kPpoMaxRowBlocks blocks, each a multiple of 64 rows
static int32_t ppo_rows_per_block(int64_t B) {
  const int64_t per = (B + kPpoMaxRowBlocks - 1) / kPpoMaxRowBlocks;
  return (int32_t)(((per + 63) / 64) * 64);
}

// scratch of minibatches of up to B rows
static int ppo_scratch(cpr_batch* b, int64_t B) {
  const PolNet& N = b->pn;
  const size_t rows = (size_t)B;
  const size_t wmax = (size_t)std::max(N.width_pi, N.width_vf);
  const size_t total = (size_t)b->pn_total;
  hipStream_t st = b->ctx->stream;
  if (b->pp_m.bytes < total * 4) {  // first use, or a larger network was set (ppo_t is 0)
    HIP_TRY(b->pp_m.ensure(total * 4));
    HIP_TRY(b->pp_v.ensure(total * 4));
    HIP_TRY(hipMemsetAsync(b->pp_m.p, 0, b->pp_m.bytes, st));
    HIP_TRY(hipMemsetAsync(b->pp_v.p, 0, b->pp_v.bytes, st));
  }
  HIP_TRY(b->pp_grad.ensure(total * 4));
  // the arrays' padding is never written by k_ppo_dw: zero once, so that the summed gradient,
  // the moments and the weights keep zeros there
  const size_t part = total * 4 * kPpoMaxRowBlocks;
  if (b->pp_part.bytes < part) {
    HIP_TRY(b->pp_part.ensure(part));
    HIP_TRY(hipMemsetAsync(b->pp_part.p, 0, part, st));
  }
  size_t biases = 0;
  for (size_t k = 1; k < b->pn_cnt.size(); k += 2) biases += (size_t)b->pn_cnt[k];
  HIP_TRY(b->pp_bpart.ensure(biases * 8 * kPpoMaxRowBlocks));
  HIP_TRY(b->pp_xin.ensure(rows * kPolInStride * 4));
  HIP_TRY(b->pp_act.ensure(rows * (size_t)N.depth * (size_t)(N.width_pi + N.width_vf) * 4));
  HIP_TRY(b->pp_dy0.ensure(2 * rows * wmax * 4));
  HIP_TRY(b->pp_dy1.ensure(2 * rows * wmax * 4));
  HIP_TRY(b->pp_dlg.ensure(rows * (size_t)N.n_actions * 4));
  HIP_TRY(b->pp_dv.ensure(rows * 4));
  HIP_TRY(b->pp_advn.ensure(rows * 8));
  HIP_TRY(b->pp_partial.ensure(((rows + kPolRows - 1) / kPolRows) * kPpoRowStats * 8));
  HIP_TRY(b->pp_stats.ensure(2 * kPpoStats * 8));  // the minibatch's, then the update's sums
  HIP_TRY(b->pp_red.ensure(3 * kPpoRedBlocks * 8));  // partials of the f64 reductions
  return CPR_OK;
}

// what a training forward leaves for the backward: the f32 input rows, each trunk's saved
// activations and the loss's derivative at the heads. pi_only (Q-learning): the vf trunk's
// jobs are empty and only the pi part of `grad` is written
struct PpoBack {
  const float* xin;
  float* const* act[2];
  const float* dlogits;
  const float* dvalue;
  bool pi_only;
  float* grad;
};
static int ppo_backward(cpr_batch* b, int64_t B, const PpoBack& K, double* acc);

// the gradient of minibatch idx[0 .. B) into pp_grad and its statistics into pp_stats (added
// to acc if given); launches only
static int ppo_minibatch(cpr_batch* b, const PpoDev& D, const int32_t* idx, int64_t B,
                         const cpr_ppo_opts& o, double* acc) {
  const PolNet& N = b->pn;
  hipStream_t st = b->ctx->stream;
  double* stats = (double*)b->pp_stats.p;
  double* red = (double*)b->pp_red.p;
  HIP_TRY(launch_adv_norm(D.adv, idx, B, D.n, o.normalize_advantage, red, (double*)b->pp_advn.p, st));
  PpoFwd F = {};
  F.obs = D.obs;
  F.alpha = D.alpha;
  F.alpha_col = D.alpha_col;
  F.action = D.action;
  F.old_logp = D.old_logp;
  F.ret = D.ret;
  F.advn = (const double*)b->pp_advn.p;
  F.idx = idx;
  F.B = B;
  F.N = D.n;
  F.clip = o.clip_range;
  F.ent_coef = o.ent_coef;
  F.vf_coef = o.vf_coef;
  F.xin = (float*)b->pp_xin.p;
  float* ap = (float*)b->pp_act.p;
  for (int trunk = 0; trunk < 2; trunk++)
    for (int l = 0; l < N.depth; l++) {
      F.act[trunk][l] = ap;
      ap += (size_t)B * (size_t)(trunk == 0 ? N.width_pi : N.width_vf);
    }
  F.dlogits = (float*)b->pp_dlg.p;
  F.dvalue = (float*)b->pp_dv.p;
  F.partial = (double*)b->pp_partial.p;
  HIP_TRY(launch_ppo_forward(N, F, st));
  const int64_t blocks = (B + kPolRows - 1) / kPolRows;
  HIP_TRY(launch_ppo_stats(F.partial, blocks, B, o.ent_coef, o.vf_coef, stats, acc, st));
  PpoBack K = {};
  K.xin = F.xin;
  K.act[0] = F.act[0];
  K.act[1] = F.act[1];
  K.dlogits = F.dlogits;
  K.dvalue = F.dvalue;
  K.grad = (float*)b->pp_grad.p;
  return ppo_backward(b, B, K, acc);
}

// backward from each head down (both trunks' layer l in one launch), the row blocks'
// partials summed into K.grad, and its norm into pp_stats (added to acc if given)
static int ppo_backward(cpr_batch* b, int64_t B, const PpoBack& K, double* acc) {
  const PolNet& N = b->pn;
  hipStream_t st = b->ctx->stream;
  double* stats = (double*)b->pp_stats.p;
  double* red = (double*)b->pp_red.p;
  PpoBwd P = {};
  P.B = B;
  P.rows_per_block = ppo_rows_per_block(B);
  P.part = (float*)b->pp_part.p;
  P.pstride = b->pn_total;
  // the biases alone, in array order: their partials are f64
  PpoBiasMap M = {};
  M.arrays = 2 * (N.depth + 1);
  for (int k = 0; k < M.arrays; k++) {
    M.off[k] = b->pn_off[2 * k + 1];
    M.start[k + 1] = M.start[k] + b->pn_cnt[2 * k + 1];
  }
  P.bpart = (double*)b->pp_bpart.p;
  P.bstride = M.start[M.arrays];
  const size_t wmax = (size_t)std::max(N.width_pi, N.width_vf);
  float* dy[2] = {(float*)b->pp_dy0.p, (float*)b->pp_dy1.p};
  const float* cur[2] = {K.dlogits, K.dvalue};
  int32_t ld[2] = {N.n_actions, 1};
  const int trunks = K.pi_only ? 1 : 2;  // P.j[1] stays empty: no tile, no dX
  for (int l = N.depth; l >= 0; l--) {
    float* out = dy[(N.depth - l) & 1];
    for (int trunk = 0; trunk < trunks; trunk++) {
      const PolLayer& Ly = trunk == 0 ? N.pi[l] : N.vf[l];
      PpoBwdJob& J = P.j[trunk];
      J.dY = cur[trunk];
      J.ldy = ld[trunk];
      J.X = l == 0 ? K.xin : K.act[trunk][l - 1];
      J.ldx = l == 0 ? kPolInStride : Ly.n_in;
      J.W = Ly.W;
      J.n_out = Ly.n_out;
      J.n_in = Ly.n_in;
      J.dX = l == 0 ? nullptr : out + (size_t)trunk * (size_t)B * wmax;
      const size_t a = (size_t)trunk * (size_t)(N.depth + 1) * 2 + (size_t)l * 2;
      J.off_w = b->pn_off[a];
      J.off_b = b->pn_off[a + 1];
      J.off_bc = M.start[a / 2];
    }
    HIP_TRY(launch_ppo_dw(P, st));
    if (l > 0) {
      HIP_TRY(launch_ppo_dx(P, st));
      for (int trunk = 0; trunk < trunks; trunk++) {
        cur[trunk] = P.j[trunk].dX;
        ld[trunk] = P.j[trunk].n_in;
      }
    }
  }
  const int32_t rb = (int32_t)((B + P.rows_per_block - 1) / P.rows_per_block);
  // the pi trunk's arrays stand first in the layout
  const int64_t n_red = K.pi_only ? b->pn_off[(size_t)2 * (N.depth + 1)] : b->pn_total;
  if (K.pi_only) M.arrays = N.depth + 1;
  HIP_TRY(launch_ppo_reduce(P.part, P.pstride, rb, n_red, K.grad, st));
  HIP_TRY(launch_ppo_reduce_bias(P.bpart, P.bstride, rb, M, K.grad, st));
  HIP_TRY(launch_grad_norm(K.grad, b->pn_total, red + 2 * kPpoRedBlocks, stats, acc, st));
  return CPR_OK;
}

static void ppo_stats_out(const double* s, double div, int64_t count, cpr_ppo_stats* out) {
  out->policy_loss = s[kPpoPolicyLoss] / div;
  out->value_loss = s[kPpoValueLoss] / div;
  out->entropy_loss = s[kPpoEntropyLoss] / div;
  out->approx_kl = s[kPpoApproxKl] / div;
  out->clip_fraction = s[kPpoClipFraction] / div;
  out->loss = s[kPpoLoss] / div;
  out->grad_norm = s[kPpoGradNorm] / div;
  out->n_minibatches = count;
}

int cpr_ppo_param_count(cpr_batch* b, int64_t* count) {
  if (!b || !count) return fail(CPR_E_INVALID_ARG, "NULL argument");
  CPR_ENTER(b->ctx);
  if (!b->has_net) return fail(CPR_E_STATE, "no policy network set (cpr_policy_net_set)");
  int64_t c = 0;
  for (int64_t k : b->pn_cnt) c += k;
  *count = c;
  return CPR_OK;
}

int cpr_ppo_gradients(cpr_batch* b, const cpr_ppo_data* data, const int32_t* rows_idx,
                      int64_t n_rows, const cpr_ppo_opts* opts, float* grad_out,
                      cpr_ppo_stats* stats_out) {
  int rc = ppo_check(b, opts);
  if (rc) return rc;
  CPR_ENTER(b->ctx);
  if (!rows_idx || !grad_out) return fail(CPR_E_INVALID_ARG, "NULL argument");
  if (n_rows < 1 || n_rows > INT32_MAX)
    return fail(CPR_E_INVALID_ARG, "ppo: n_rows must be in 1 .. 2^31 - 1");
  PpoDev D;
  rc = ppo_stage(b, data, &D);
  if (rc) return rc;
  hipStream_t st = b->ctx->stream;
  const int32_t* idx = rows_idx;
  if (!data->on_device) {
    for (int64_t i = 0; i < n_rows; i++)
      if (rows_idx[i] < 0 || rows_idx[i] >= D.n)
        return fail(CPR_E_INVALID_ARG, "ppo: rows_idx out of range");
    HIP_TRY(b->pp_idx.ensure((size_t)n_rows * 4));
    HIP_TRY(hipMemcpyAsync(b->pp_idx.p, rows_idx, (size_t)n_rows * 4, hipMemcpyHostToDevice, st));
    idx = (const int32_t*)b->pp_idx.p;
  }
  rc = ppo_scratch(b, n_rows);
  if (rc) return rc;
  rc = ppo_minibatch(b, D, idx, n_rows, *opts, nullptr);
  if (rc) return rc;
  float* g = grad_out;
  for (size_t i = 0; i < b->pn_cnt.size(); i++) {
    HIP_TRY(hipMemcpyAsync(g, (const float*)b->pp_grad.p + b->pn_off[i], (size_t)b->pn_cnt[i] * 4,
                           hipMemcpyDeviceToHost, st));
    g += b->pn_cnt[i];
  }
  double s[kPpoStats];
  HIP_TRY(hipMemcpyAsync(s, b->pp_stats.p, sizeof(s), hipMemcpyDeviceToHost, st));
  HIP_TRY(hipStreamSynchronize(st));
  if (stats_out) ppo_stats_out(s, 1.0, 1, stats_out);
  return CPR_OK;
}

// epoch e's permutation of 0 .. n - 1 (include/cpr_hip.h cpr_ppo_update)
constexpr uint32_t TAG_PERM = 0x80000000u;
static void ppo_draw_perm(uint64_t seed, uint64_t perm_seed, uint64_t update, uint32_t epoch,
                          int64_t n, int32_t* p) {
  const uint64_t key = seed ^ (perm_seed * 0x9E3779B97F4A7C15ull);
  for (int64_t i = 0; i < n; i++) p[i] = (int32_t)i;
  Words4 w = {};
  int64_t have = -1;
  for (int64_t i = n - 1; i >= 1; i--) {
    if (have != (i >> 1)) {
      have = i >> 1;
      w = philox4x32_10((uint32_t)update, epoch, (uint32_t)have, TAG_PERM, (uint32_t)key,
                        (uint32_t)(key >> 32));
    }
    const double u = (i & 1) ? u53(w.w2, w.w3) : u53(w.w0, w.w1);
    int64_t j = (int64_t)(u * (double)(i + 1));
    if (j > i) j = i;
    std::swap(p[i], p[j]);
  }
}

int cpr_ppo_update(cpr_batch* b, const cpr_ppo_data* data, const cpr_ppo_opts* opts,
                   const int32_t* perm, cpr_ppo_stats* stats_out) {
  int rc = ppo_check(b, opts);
  if (rc) return rc;
  CPR_ENTER(b->ctx);
  PpoDev D;
  rc = ppo_stage(b, data, &D);
  if (rc) return rc;
  const cpr_ppo_opts& o = *opts;
  hipStream_t st = b->ctx->stream;
  const int64_t n = D.n;
  const size_t cells = (size_t)o.n_epochs * (size_t)n;
  const int32_t* pd = perm;
  if (!perm || !data->on_device) {
    if (perm) {
      for (size_t i = 0; i < cells; i++)
        if (perm[i] < 0 || perm[i] >= n) return fail(CPR_E_INVALID_ARG, "ppo: perm out of range");
    } else {
      // drawn here, uploaded behind the kernels already queued; perm_host stays until the
      // synchronisation at the end of this call
      b->perm_host.resize(cells);
      for (int32_t e = 0; e < o.n_epochs; e++)
        ppo_draw_perm(b->cfg.seed, o.perm_seed, (uint64_t)b->ppo_updates, (uint32_t)e, n,
                      b->perm_host.data() + (size_t)e * (size_t)n);
    }
    HIP_TRY(b->pp_perm.ensure(cells * 4));
    HIP_TRY(hipMemcpyAsync(b->pp_perm.p, perm ? perm : b->perm_host.data(), cells * 4,
                           hipMemcpyHostToDevice, st));
    pd = (const int32_t*)b->pp_perm.p;
  }
  const int64_t mb = std::min<int64_t>(o.minibatch, n);
  rc = ppo_scratch(b, mb);
  if (rc) return rc;
  double* acc = (double*)b->pp_stats.p + kPpoStats;
  HIP_TRY(hipMemsetAsync(acc, 0, kPpoStats * 8, st));
  int64_t count = 0;
  for (int32_t e = 0; e < o.n_epochs; e++)
    for (int64_t s0 = 0; s0 < n; s0 += mb) {
      const int64_t B = std::min<int64_t>(mb, n - s0);
      rc = ppo_minibatch(b, D, pd + (size_t)e * (size_t)n + s0, B, o, acc);
      if (rc) return rc;
      const double t = (double)++b->ppo_t;
      PpoAdam A = {};
      A.p = (float*)b->pn_w.p;
      A.g = (const float*)b->pp_grad.p;
      A.m = (float*)b->pp_m.p;
      A.v = (float*)b->pp_v.p;
      A.n = b->pn_total;
      A.stats = (const double*)b->pp_stats.p;
      A.max_norm = (float)o.max_grad_norm;
      A.b1 = (float)o.beta1;
      A.omb1 = (float)(1.0 - o.beta1);
      A.b2 = (float)o.beta2;
      A.omb2 = (float)(1.0 - o.beta2);
      A.step = (float)(o.lr / (1.0 - std::pow(o.beta1, t)));
      A.bc2_sqrt = (float)std::sqrt(1.0 - std::pow(o.beta2, t));
      A.eps = (float)o.adam_eps;
      HIP_TRY(launch_adam(A, st));
      ++count;
    }
  double s[kPpoStats];
  HIP_TRY(hipMemcpyAsync(s, acc, sizeof(s), hipMemcpyDeviceToHost, st));
  HIP_TRY(hipStreamSynchronize(st));
  ++b->ppo_updates;
  if (stats_out) ppo_stats_out(s, (double)count, count, stats_out);
  return CPR_OK;
}

int cpr_ppo_iterate(cpr_batch* b, int64_t n_steps, const cpr_ppo_opts* opts,
                    cpr_summary* summary, cpr_ppo_stats* stats_out) {
  int rc = ppo_check(b, opts);
  if (rc) return rc;
  CPR_ENTER(b->ctx);
  if (!summary) return fail(CPR_E_INVALID_ARG, "NULL argument");
  if (n_steps < 1) return fail(CPR_E_INVALID_ARG, "ppo: n_steps must be >= 1");
  const int64_t n = b->cfg.n_lanes;
  if (n_steps * n > INT32_MAX)
    return fail(CPR_E_INVALID_ARG, "ppo: n_steps * n_lanes above 2^31 - 1 (int32 rows)");
  const size_t cells = (size_t)(n_steps * n);
  const size_t ol = (size_t)obs_len_of(b->cfg);
  // obs0 and obs share one buffer, so that the policy input of flat row r is its row r; the
  // same for the alphas
  HIP_TRY(b->it_obs.ensure((cells + (size_t)n) * ol * 8));
  HIP_TRY(b->it_alpha.ensure((cells + (size_t)n) * 8));
  HIP_TRY(b->it_action.ensure(cells * 4));
  HIP_TRY(b->it_reward.ensure(cells * 8));
  HIP_TRY(b->it_done.ensure(cells));
  HIP_TRY(b->it_logp.ensure(cells * 8));
  HIP_TRY(b->it_value.ensure((cells + (size_t)n) * 8));
  HIP_TRY(b->it_adv.ensure(cells * 8));
  HIP_TRY(b->it_ret.ensure(cells * 8));
  cpr_rollout_net_out out = {};
  out.obs0 = (double*)b->it_obs.p;
  out.obs = out.obs0 + (size_t)n * ol;
  out.action = (int32_t*)b->it_action.p;
  out.reward = (double*)b->it_reward.p;
  out.done = (uint8_t*)b->it_done.p;
  out.logp = (double*)b->it_logp.p;
  out.value = (double*)b->it_value.p;
  cpr_rollout_env_out eo = {};
  eo.alpha0 = (double*)b->it_alpha.p;
  eo.alpha = eo.alpha0 + n;
  rc = cpr_rollout_net_env(b, n_steps, 0, &out, &eo, 1, summary);
  if (rc) return rc;
  rc = cpr_gae(b, n_steps, out.reward, out.done, out.value, opts->gae_gamma, opts->gae_lambda,
               (double*)b->it_adv.p, (double*)b->it_ret.p, 1);
  if (rc) return rc;
  cpr_ppo_data d = {};
  d.n = (int64_t)cells;
  d.obs = out.obs0;
  d.alpha = eo.alpha0;
  d.action = out.action;
  d.old_logp = out.logp;
  d.advantage = (const double*)b->it_adv.p;
  d.ret = (const double*)b->it_ret.p;
  d.on_device = 1;
  return cpr_ppo_update(b, &d, opts, nullptr, stats_out);
}

// ---------------------------------------------------------------- Q-learning (dqn.h)

int cpr_dqn_opts_default(cpr_dqn_opts* o) {
  if (!o) return fail(CPR_E_INVALID_ARG, "NULL argument");
  *o = cpr_dqn_opts{};
  o->batch = 32;
  o->gradient_steps = 1;
  o->gamma = 0.99;
  o->lr = 1e-4;
  o->beta1 = 0.9;
  o->beta2 = 0.999;
  o->adam_eps = 1e-8;
  o->max_grad_norm = 10.0;
  o->tau = 1.0;
  o->target_update_interval = 10000;
  o->learning_starts = 50000;
  o->sample_seed = 0;
  return CPR_OK;
}

// the batch can hold a Q-network at all, and holds one (and a ring, if asked for)
static int dqn_state(cpr_batch* b, bool need_ring) {
  if (!b) return fail(CPR_E_INVALID_ARG, "NULL argument");
  if (b->cfg.protocol == CPR_PROTO_FC16)
    return fail(CPR_E_UNSUPPORTED, "FC16 runs fused episodes (cpr_run_episodes) only");
  if (b->cfg.n_lanes <= 0 || b->cfg.mode != CPR_MODE_GYM)
    return fail(CPR_E_UNSUPPORTED, "Q-learning needs lockstep lanes (CPR_MODE_GYM, "
                                   "cfg.n_lanes > 0)");
  if (!b->has_net) return fail(CPR_E_STATE, "no policy network set (cpr_policy_net_set)");
  if (need_ring && !b->dq_ready) return fail(CPR_E_STATE, "no replay ring (cpr_dqn_init)");
  return CPR_OK;
}

// state, shapes and options of the cpr_dqn_* calls that take options, before any launch
static int dqn_check(cpr_batch* b, const cpr_dqn_opts* o) {
  int rc = dqn_state(b, true);
  if (rc) return rc;
  if (!o) return fail(CPR_E_INVALID_ARG, "NULL argument");
  if (o->batch < 1) return fail(CPR_E_INVALID_ARG, "dqn: batch must be >= 1");
  if (o->batch > INT32_MAX) return fail(CPR_E_INVALID_ARG, "dqn: batch above 2^31 - 1");
  if (o->gradient_steps < 0) return fail(CPR_E_INVALID_ARG, "dqn: gradient_steps must be >= 0");
  if (o->target_update_interval < 1)
    return fail(CPR_E_INVALID_ARG, "dqn: target_update_interval must be >= 1");
  if (o->learning_starts < 0) return fail(CPR_E_INVALID_ARG, "dqn: learning_starts must be >= 0");
  const struct {
    const char* name;
    double v;
    bool positive;
  } fields[] = {{"gamma", o->gamma, false},       {"lr", o->lr, false},
                {"beta1", o->beta1, false},       {"beta2", o->beta2, false},
                {"adam_eps", o->adam_eps, false}, {"max_grad_norm", o->max_grad_norm, true},
                {"tau", o->tau, false}};
  for (const auto& f : fields) {
    if (!std::isfinite(f.v)) return fail(CPR_E_INVALID_ARG, std::string("dqn: non-finite ") + f.name);
    if (f.positive && !(f.v > 0.0))
      return fail(CPR_E_INVALID_ARG, std::string("dqn: ") + f.name + " must be > 0");
  }
  if (!(o->beta1 >= 0.0 && o->beta1 < 1.0) || !(o->beta2 >= 0.0 && o->beta2 < 1.0))
    return fail(CPR_E_INVALID_ARG, "dqn: beta1 and beta2 must be in [0, 1)");
  if (!(o->tau >= 0.0 && o->tau <= 1.0)) return fail(CPR_E_INVALID_ARG, "dqn: tau must be in [0, 1]");
  HIP_TRY(hipSetDevice(b->ctx->device));
  const int64_t lds = policy_lds_bytes(b->pn.depth, b->pn.width_pi, b->pn.width_vf);
  if (lds > dqn_lds_limit())
    return fail(CPR_E_UNSUPPORTED,
                "dqn: the forward of this network needs " + std::to_string(lds) +
                    " B of LDS per workgroup, the device has " + std::to_string(dqn_lds_limit()));
  return CPR_OK;
}

int cpr_dqn_init(cpr_batch* b, int64_t capacity_steps) {
  int rc = dqn_state(b, false);
  if (rc) return rc;
  CPR_ENTER(b->ctx);
  if (capacity_steps < 1) return fail(CPR_E_INVALID_ARG, "dqn: capacity_steps must be >= 1");
  const int64_t n = b->cfg.n_lanes;
  if (capacity_steps > (INT64_MAX >> 8) / n)
    return fail(CPR_E_INVALID_ARG, "dqn: capacity_steps * n_lanes overflows");
  HIP_TRY(hipSetDevice(b->ctx->device));
  hipStream_t st = b->ctx->stream;
  HIP_TRY(hipStreamSynchronize(st));  // a kernel may still be reading a previous ring
  b->dq_ready = false;
  // the ring and its guard slot; a failed allocation leaves the batch without a ring
  const size_t rows = (size_t)(capacity_steps + 1) * (size_t)n, ol = (size_t)b->pn.obs_len;
  struct {
    DevBuf* buf;
    size_t bytes;
  } arrs[] = {{&b->dq_obs, rows * ol * 4}, {&b->dq_next, rows * ol * 4}, {&b->dq_alpha, rows * 8},
              {&b->dq_action, rows * 4},   {&b->dq_reward, rows * 8},    {&b->dq_done, rows}};
  for (auto& a : arrs) {
    a.buf->release();
    HIP_TRY(a.buf->ensure(a.bytes));
  }
  for (auto& a : arrs) {
    const size_t ring = a.bytes / (size_t)(capacity_steps + 1) * (size_t)capacity_steps;
    HIP_TRY(hipMemsetAsync(a.buf->p, 0, ring, st));
    HIP_TRY(hipMemsetAsync((char*)a.buf->p + ring, 0xA5, a.bytes - ring, st));
  }
  b->dq_cap = capacity_steps;
  b->dq_cursor = 0;
  b->dq_size = 0;
  b->dq_steps = 0;
  b->dq_idx_n = 0;
  b->ppo_t = 0;
  if (b->pp_m.p) HIP_TRY(hipMemsetAsync(b->pp_m.p, 0, b->pp_m.bytes, st));
  if (b->pp_v.p) HIP_TRY(hipMemsetAsync(b->pp_v.p, 0, b->pp_v.bytes, st));
  rc = dqn_target_reset(b);
  if (rc) return rc;
  HIP_TRY(hipStreamSynchronize(st));
  b->dq_ready = true;
  return CPR_OK;
}

int cpr_dqn_collect(cpr_batch* b, int64_t n_steps, double epsilon, cpr_summary* summary) {
  int rc = dqn_state(b, true);
  if (rc) return rc;
  if (!(epsilon >= 0.0 && epsilon <= 1.0))
    return fail(CPR_E_INVALID_ARG, "dqn: epsilon must be in [0, 1]");
  if (n_steps < 0) return fail(CPR_E_INVALID_ARG, "dqn: n_steps must be >= 0");
  return rollout_net_run(b, n_steps, 1, nullptr, nullptr, 1, summary, &epsilon);
}

int cpr_dqn_replay_state(cpr_batch* b, int64_t* size, int64_t* cursor, int64_t* capacity) {
  int rc = dqn_state(b, true);
  if (rc) return rc;
  if (size) *size = b->dq_size;
  if (cursor) *cursor = b->dq_cursor;
  if (capacity) *capacity = b->dq_cap;
  return CPR_OK;
}

int cpr_dqn_replay_get(cpr_batch* b, int64_t first_slot, int64_t n_slots, cpr_dqn_data* out) {
  int rc = dqn_state(b, true);
  if (rc) return rc;
  CPR_ENTER(b->ctx);
  if (!out || !out->obs || !out->action || !out->reward || !out->done || !out->next_obs)
    return fail(CPR_E_INVALID_ARG, "NULL argument");
  if (first_slot < 0 || n_slots < 1 || first_slot > b->dq_cap || n_slots > b->dq_cap + 1 - first_slot)
    return fail(CPR_E_INVALID_ARG, "dqn: slots outside the ring and its guard slot");
  HIP_TRY(hipSetDevice(b->ctx->device));
  hipStream_t st = b->ctx->stream;
  const size_t rows = (size_t)n_slots * (size_t)b->cfg.n_lanes, ol = (size_t)b->pn.obs_len;
  const DqnRows S = dqn_slot(b, first_slot);
  std::vector<float> o32(rows * ol), n32(rows * ol);
  HIP_TRY(hipMemcpyAsync(o32.data(), S.obs, rows * ol * 4, hipMemcpyDeviceToHost, st));
  HIP_TRY(hipMemcpyAsync(n32.data(), S.next_obs, rows * ol * 4, hipMemcpyDeviceToHost, st));
  if (out->alpha)
    HIP_TRY(hipMemcpyAsync((void*)out->alpha, S.alpha, rows * 8, hipMemcpyDeviceToHost, st));
  HIP_TRY(hipMemcpyAsync((void*)out->action, S.action, rows * 4, hipMemcpyDeviceToHost, st));
  HIP_TRY(hipMemcpyAsync((void*)out->reward, S.reward, rows * 8, hipMemcpyDeviceToHost, st));
  HIP_TRY(hipMemcpyAsync((void*)out->done, S.done, rows, hipMemcpyDeviceToHost, st));
  HIP_TRY(hipStreamSynchronize(st));
  for (size_t i = 0; i < rows * ol; i++) {
    ((double*)out->obs)[i] = (double)o32[i];
    ((double*)out->next_obs)[i] = (double)n32[i];
  }
  out->n = (int64_t)rows;
  out->on_device = 0;
  return CPR_OK;
}

static int policy_net_read(cpr_batch* b, const void* weights, cpr_policy_net* net);

int cpr_dqn_target_get(cpr_batch* b, cpr_policy_net* net) {
  int rc = dqn_state(b, true);
  if (rc) return rc;
  if (!net) return fail(CPR_E_INVALID_ARG, "NULL argument");
  CPR_ENTER(b->ctx);
  return policy_net_read(b, b->dq_tw.p, net);
}

// the gradient of the transitions idx[0 .. B) of F's rows into dq_grad and the step's
// statistics into pp_stats (added to acc if given); launches only
static int dqn_minibatch(cpr_batch* b, DqnFwd F, const int64_t* idx, int64_t B, double* acc) {
  const PolNet& N = b->pn;
  hipStream_t st = b->ctx->stream;
  F.idx = idx;
  F.B = B;
  F.xin = (float*)b->pp_xin.p;
  float* ap = (float*)b->pp_act.p;
  for (int l = 0; l < N.depth; l++) {
    F.act[l] = ap;
    ap += (size_t)B * (size_t)N.width_pi;
  }
  F.dlogits = (float*)b->pp_dlg.p;
  F.partial = (double*)b->pp_partial.p;
  HIP_TRY(launch_dqn_forward(N, b->dq_tn, F, st));
  const int64_t blocks = (B + kPolRows - 1) / kPolRows;
  HIP_TRY(launch_dqn_stats(F.partial, blocks, B, (double*)b->pp_stats.p, acc, st));
  PpoBack K = {};
  K.xin = F.xin;
  K.act[0] = F.act;
  K.dlogits = F.dlogits;
  K.pi_only = true;
  K.grad = (float*)b->dq_grad.p;
  return ppo_backward(b, B, K, acc);
}

static void dqn_stats_out(const double* s, double div, int64_t count, cpr_dqn_stats* out) {
  out->loss = s[kDqnLoss] / div;
  out->abs_td = s[kDqnAbsTd] / div;
  out->q = s[kDqnQ] / div;
  out->target = s[kDqnTarget] / div;
  out->grad_norm = s[kPpoGradNorm] / div;
  out->n_steps = count;
}

int cpr_dqn_gradients(cpr_batch* b, const cpr_dqn_data* data, const int64_t* rows_idx,
                      int64_t n_rows, const cpr_dqn_opts* opts, float* grad_out,
                      cpr_dqn_stats* stats_out) {
  int rc = dqn_check(b, opts);
  if (rc) return rc;
  CPR_ENTER(b->ctx);
  if (!data || !rows_idx || !grad_out) return fail(CPR_E_INVALID_ARG, "NULL argument");
  if (n_rows < 1 || n_rows > INT32_MAX)
    return fail(CPR_E_INVALID_ARG, "dqn: n_rows must be in 1 .. 2^31 - 1");
  if (data->n < 1) return fail(CPR_E_INVALID_ARG, "dqn: data.n must be >= 1");
  if (!data->obs || !data->action || !data->reward || !data->done || !data->next_obs)
    return fail(CPR_E_INVALID_ARG, "dqn: NULL data array");
  const bool use_alpha = b->has_env && b->env.alpha_column >= 0;
  if (use_alpha && !data->alpha)
    return fail(CPR_E_INVALID_ARG, "dqn: data.alpha is NULL but the lane env names an alpha column");
  hipStream_t st = b->ctx->stream;
  DqnFwd F = {};
  F.N = data->n;
  F.gamma = opts->gamma;
  F.alpha_col = use_alpha ? b->env.alpha_column : -1;
  const int64_t* idx = rows_idx;
  if (data->on_device) {
    F.obs64 = data->obs;
    F.next64 = data->next_obs;
    F.alpha = use_alpha ? data->alpha : nullptr;
    F.action = data->action;
    F.reward = data->reward;
    F.done = data->done;
  } else {
    const size_t n = (size_t)data->n, ol = (size_t)b->pn.obs_len;
    for (size_t i = 0; i < n; i++)
      if (data->action[i] < 0 || data->action[i] >= b->pn.n_actions)
        return fail(CPR_E_INVALID_ARG, "dqn: data.action out of range");
    for (int64_t i = 0; i < n_rows; i++)
      if (rows_idx[i] < 0 || rows_idx[i] >= data->n)
        return fail(CPR_E_INVALID_ARG, "dqn: rows_idx out of range");
    struct {
      DevBuf* buf;
      const void* src;
      size_t bytes;
    } cp[] = {{&b->ds_obs, data->obs, n * ol * 8},
              {&b->ds_next, data->next_obs, n * ol * 8},
              {&b->ds_alpha, use_alpha ? data->alpha : nullptr, n * 8},
              {&b->ds_action, data->action, n * 4},
              {&b->ds_reward, data->reward, n * 8},
              {&b->ds_done, data->done, n},
              {&b->ds_idx, rows_idx, (size_t)n_rows * 8}};
    for (auto& c : cp) {
      if (!c.src) continue;
      HIP_TRY(c.buf->ensure(c.bytes));
      HIP_TRY(hipMemcpyAsync(c.buf->p, c.src, c.bytes, hipMemcpyHostToDevice, st));
    }
    F.obs64 = (const double*)b->ds_obs.p;
    F.next64 = (const double*)b->ds_next.p;
    F.alpha = use_alpha ? (const double*)b->ds_alpha.p : nullptr;
    F.action = (const int32_t*)b->ds_action.p;
    F.reward = (const double*)b->ds_reward.p;
    F.done = (const uint8_t*)b->ds_done.p;
    idx = (const int64_t*)b->ds_idx.p;
  }
  rc = ppo_scratch(b, n_rows);
  if (rc) return rc;
  rc = dqn_minibatch(b, F, idx, n_rows, nullptr);
  if (rc) return rc;
  float* g = grad_out;
  for (size_t i = 0; i < b->pn_cnt.size(); i++) {
    HIP_TRY(hipMemcpyAsync(g, (const float*)b->dq_grad.p + b->pn_off[i], (size_t)b->pn_cnt[i] * 4,
                           hipMemcpyDeviceToHost, st));
    g += b->pn_cnt[i];
  }
  double s[kPpoStats];
  HIP_TRY(hipMemcpyAsync(s, b->pp_stats.p, sizeof(s), hipMemcpyDeviceToHost, st));
  HIP_TRY(hipStreamSynchronize(st));
  if (stats_out) dqn_stats_out(s, 1.0, 1, stats_out);
  return CPR_OK;
}

// the indices of gradient step g of update U (include/cpr_hip.h cpr_dqn_update)
static void dqn_draw(uint64_t seed, uint64_t sample_seed, uint64_t update, uint32_t g,
                     int64_t batch, int64_t n, int64_t* out) {
  const uint64_t key = seed ^ (sample_seed * 0x9E3779B97F4A7C15ull);
  Words4 w = {};
  for (int64_t i = 0; i < batch; i++) {
    if ((i & 1) == 0)
      w = philox4x32_10((uint32_t)update, g, (uint32_t)(i >> 1), TAG_REPLAY, (uint32_t)key,
                        (uint32_t)(key >> 32));
    const double u = (i & 1) ? u53(w.w2, w.w3) : u53(w.w0, w.w1);
    const int64_t j = (int64_t)(u * (double)n);
    out[i] = j < n - 1 ? j : n - 1;
  }
}

int cpr_dqn_update(cpr_batch* b, int32_t gradient_steps, const cpr_dqn_opts* opts,
                   const int64_t* idx, cpr_dqn_stats* stats_out) {
  int rc = dqn_check(b, opts);
  if (rc) return rc;
  CPR_ENTER(b->ctx);
  if (gradient_steps < 0) return fail(CPR_E_INVALID_ARG, "dqn: gradient_steps must be >= 0");
  if (b->dq_size < 1) return fail(CPR_E_STATE, "dqn: the replay ring is empty (cpr_dqn_collect)");
  const cpr_dqn_opts& o = *opts;
  hipStream_t st = b->ctx->stream;
  const int64_t n = b->dq_size * b->cfg.n_lanes, B = o.batch;
  const size_t cells = (size_t)gradient_steps * (size_t)B;
  if (stats_out) *stats_out = cpr_dqn_stats{};
  if (gradient_steps == 0) return CPR_OK;
  if (idx) {
    for (size_t i = 0; i < cells; i++)
      if (idx[i] < 0 || idx[i] >= n)
        return fail(CPR_E_INVALID_ARG, "dqn: idx outside the ring's written transitions");
  } else {
    // drawn here, uploaded behind the kernels already queued; dq_idx_host stays until the
    // synchronisation at the end of this call
    b->dq_idx_host.resize(cells);
    for (int32_t g = 0; g < gradient_steps; g++)
      dqn_draw(b->cfg.seed, o.sample_seed, (uint64_t)b->dq_updates, (uint32_t)g, B, n,
               b->dq_idx_host.data() + (size_t)g * (size_t)B);
  }
  HIP_TRY(b->dq_idx.ensure(cells * 8));
  HIP_TRY(hipMemcpyAsync(b->dq_idx.p, idx ? idx : b->dq_idx_host.data(), cells * 8,
                         hipMemcpyHostToDevice, st));
  b->dq_idx_n = (int64_t)cells;
  rc = ppo_scratch(b, B);
  if (rc) return rc;
  const DqnRows R = dqn_slot(b, 0);
  DqnFwd F = {};
  F.obs32 = R.obs;
  F.next32 = R.next_obs;
  F.alpha = R.alpha;
  F.alpha_col = b->has_env ? b->env.alpha_column : -1;
  F.action = R.action;
  F.reward = R.reward;
  F.done = R.done;
  F.N = n;
  F.gamma = o.gamma;
  double* acc = (double*)b->pp_stats.p + kPpoStats;
  HIP_TRY(hipMemsetAsync(acc, 0, kPpoStats * 8, st));
  for (int32_t g = 0; g < gradient_steps; g++) {
    rc = dqn_minibatch(b, F, (const int64_t*)b->dq_idx.p + (size_t)g * (size_t)B, B, acc);
    if (rc) return rc;
    const double t = (double)++b->ppo_t;
    PpoAdam A = {};
    A.p = (float*)b->pn_w.p;
    A.g = (const float*)b->dq_grad.p;
    A.m = (float*)b->pp_m.p;
    A.v = (float*)b->pp_v.p;
    A.n = b->pn_total;
    A.stats = (const double*)b->pp_stats.p;
    A.max_norm = (float)o.max_grad_norm;
    A.b1 = (float)o.beta1;
    A.omb1 = (float)(1.0 - o.beta1);
    A.b2 = (float)o.beta2;
    A.omb2 = (float)(1.0 - o.beta2);
    A.step = (float)(o.lr / (1.0 - std::pow(o.beta1, t)));
    A.bc2_sqrt = (float)std::sqrt(1.0 - std::pow(o.beta2, t));
    A.eps = (float)o.adam_eps;
    HIP_TRY(launch_adam(A, st));
  }
  double s[kPpoStats];
  HIP_TRY(hipMemcpyAsync(s, acc, sizeof(s), hipMemcpyDeviceToHost, st));
  HIP_TRY(hipStreamSynchronize(st));
  ++b->dq_updates;
  if (stats_out) dqn_stats_out(s, (double)gradient_steps, gradient_steps, stats_out);
  return CPR_OK;
}

int cpr_dqn_last_indices(cpr_batch* b, int64_t* out, int64_t n) {
  int rc = dqn_state(b, true);
  if (rc) return rc;
  CPR_ENTER(b->ctx);
  if (!out) return fail(CPR_E_INVALID_ARG, "NULL argument");
  if (n < 1 || n > b->dq_idx_n)
    return fail(CPR_E_INVALID_ARG, "dqn: more indices than the last update read");
  HIP_TRY(hipSetDevice(b->ctx->device));
  hipStream_t st = b->ctx->stream;
  HIP_TRY(hipMemcpyAsync(out, b->dq_idx.p, (size_t)n * 8, hipMemcpyDeviceToHost, st));
  HIP_TRY(hipStreamSynchronize(st));
  return CPR_OK;
}

int cpr_dqn_target_sync(cpr_batch* b, double tau) {
  int rc = dqn_state(b, true);
  if (rc) return rc;
  CPR_ENTER(b->ctx);
  if (!(tau >= 0.0 && tau <= 1.0)) return fail(CPR_E_INVALID_ARG, "dqn: tau must be in [0, 1]");
  HIP_TRY(hipSetDevice(b->ctx->device));
  hipStream_t st = b->ctx->stream;
  HIP_TRY(launch_polyak((float*)b->dq_tw.p, (const float*)b->pn_w.p, b->pn_total,
                        (float)(1.0 - tau), (float)tau, st));
  HIP_TRY(hipStreamSynchronize(st));
  return CPR_OK;
}

int cpr_dqn_iterate(cpr_batch* b, int64_t n_steps, double epsilon, const cpr_dqn_opts* opts,
                    cpr_summary* summary, cpr_dqn_stats* stats_out) {
  int rc = dqn_check(b, opts);
  if (rc) return rc;
  if (!summary) return fail(CPR_E_INVALID_ARG, "NULL argument");
  if (n_steps < 1) return fail(CPR_E_INVALID_ARG, "dqn: n_steps must be >= 1");
  const int64_t n = b->cfg.n_lanes;
  const int64_t every = std::max<int64_t>(opts->target_update_interval / n, 1);
  const int64_t before = b->dq_steps;
  rc = cpr_dqn_collect(b, n_steps, epsilon, summary);
  if (rc) return rc;
  if (b->dq_steps / every != before / every) {
    rc = cpr_dqn_target_sync(b, opts->tau);
    if (rc) return rc;
  }
  if (stats_out) *stats_out = cpr_dqn_stats{};
  if (b->dq_steps * n < opts->learning_starts) return CPR_OK;
  return cpr_dqn_update(b, opts->gradient_steps, opts, nullptr, stats_out);
}

int cpr_policy_net_get(cpr_batch* b, cpr_policy_net* net) {
  if (!b || !net) return fail(CPR_E_INVALID_ARG, "NULL argument");
  CPR_ENTER(b->ctx);
  if (!b->has_net) return fail(CPR_E_STATE, "no policy network set (cpr_policy_net_set)");
  return policy_net_read(b, b->pn_w.p, net);
}

// a parameter buffer in the network's padded layout (the weights, or Q-learning's target) into
// the caller's arrays
static int policy_net_read(cpr_batch* b, const void* weights, cpr_policy_net* net) {
  const PolNet& N = b->pn;
  std::vector<float*> dst;
  for (int trunk = 0; trunk < 2; trunk++) {
    for (int l = 0; l < N.depth; l++) {
      dst.push_back((float*)(trunk == 0 ? net->pi_w[l] : net->vf_w[l]));
      dst.push_back((float*)(trunk == 0 ? net->pi_b[l] : net->vf_b[l]));
    }
    dst.push_back((float*)(trunk == 0 ? net->pi_head_w : net->vf_head_w));
    dst.push_back((float*)(trunk == 0 ? net->pi_head_b : net->vf_head_b));
  }
  for (float* p : dst)
    if (!p) return fail(CPR_E_INVALID_ARG, "policy net: NULL weight or bias array");
  net->n_extra = N.n_extra;
  for (int i = 0; i < N.n_extra; i++) net->extra[i] = N.extra[i];
  net->depth = N.depth;
  net->width_pi = N.width_pi;
  net->width_vf = N.width_vf;
  HIP_TRY(hipSetDevice(b->ctx->device));
  hipStream_t st = b->ctx->stream;
  for (size_t i = 0; i < dst.size(); i++)
    HIP_TRY(hipMemcpyAsync(dst[i], (const float*)weights + b->pn_off[i], (size_t)b->pn_cnt[i] * 4,
                           hipMemcpyDeviceToHost, st));
  HIP_TRY(hipStreamSynchronize(st));
  return CPR_OK;
}

int cpr_stream_fill(cpr_ctx* ctx, uint64_t seed, uint64_t ep, uint32_t idx0, uint32_t tag,
                    int64_t n, uint32_t* out, double* exp_out) {
  if (!ctx || !out) return fail(CPR_E_INVALID_ARG, "NULL argument");
  CPR_ENTER(ctx);
  if (n <= 0) return CPR_OK;
  HIP_TRY(hipSetDevice(ctx->device));
  DevBuf o, e;
  HIP_TRY(o.ensure((size_t)n * 16));
  if (exp_out) HIP_TRY(e.ensure((size_t)n * 8));
  HIP_TRY(launch_stream_fill(seed, ep, idx0, tag, n, (uint32_t*)o.p, (double*)e.p, ctx->stream));
  HIP_TRY(hipMemcpyAsync(out, o.p, (size_t)n * 16, hipMemcpyDeviceToHost, ctx->stream));
  if (exp_out)
    HIP_TRY(hipMemcpyAsync(exp_out, e.p, (size_t)n * 8, hipMemcpyDeviceToHost, ctx->stream));
  HIP_TRY(hipStreamSynchronize(ctx->stream));
  o.release();
  e.release();
  return CPR_OK;
}


int cpr_mdp_vi_opts_default(cpr_mdp_vi_opts* opts) {
  if (!opts) return fail(CPR_E_INVALID_ARG, "opts is NULL");
  opts->stop_delta = 1e-6;
  opts->discount = 1.0;
  opts->max_iter = 0;
  opts->path = CPR_MDP_VI_AUTO;
  return CPR_OK;
}

// the sweep cap of a solve with max_iter == 0: kMdpSweepCap; CPR_MDP_VI_SWEEP_CAP lowers it
// (tests reach `not converged` in a few thousand sweeps)
static int64_t mdp_sweep_cap() {
  if (const char* e = getenv("CPR_MDP_VI_SWEEP_CAP")) {
    const long long v = atoll(e);
    if (v >= 1 && v < kMdpSweepCap) return v;
  }
  return kMdpSweepCap;
}

// The checks of a cpr_mdp that both MDP entries make before anything is allocated or launched;
// a used slot is checked whether or not its action is valid (the host solver would read
// value[dst] of such a slot too)
static int mdp_check(const cpr_mdp* mdp) {
  if (mdp->S < 1 || mdp->A < 1 || mdp->T < 1 || mdp->P < 1)
    return fail(CPR_E_INVALID_ARG, "mdp: S, A, T and P must be at least 1");
  if (!mdp->dst || !mdp->used || !mdp->valid || !mdp->rew || !mdp->prg || !mdp->prb)
    return fail(CPR_E_INVALID_ARG, "mdp: NULL array");
  const int64_t S = mdp->S, A = mdp->A, T = mdp->T, P = mdp->P;
  const int64_t AT = A * T;  // < 2^62
  if (AT > ((int64_t)1 << 36) / S || AT * S > ((int64_t)1 << 36) / P)
    return fail(CPR_E_INVALID_ARG, "mdp: more than 2^36 transition slots over all points");
  const int64_t slots = AT * S;
  for (int64_t i = 0; i < slots; ++i) {
    if (!mdp->used[i]) continue;
    if (mdp->dst[i] < 0 || mdp->dst[i] >= S)
      return fail(CPR_E_INVALID_ARG, "mdp: a used slot's dst is outside [0, S)");
    if (!std::isfinite(mdp->rew[i]) || !std::isfinite(mdp->prg[i]))
      return fail(CPR_E_INVALID_ARG, "mdp: a used slot's rew or prg is not finite");
    for (int64_t p = 0; p < P; ++p)
      if (!std::isfinite(mdp->prb[p * slots + i]))
        return fail(CPR_E_INVALID_ARG, "mdp: a used slot's prb is not finite");
  }
  return CPR_OK;
}

// A checked cpr_mdp on the device in the kernels' layout: state index fastest, unused slots
// marked by dst = -1. The host copies live as long as the device ones.
struct MdpUpload {
  std::vector<int32_t> dst_t;
  std::vector<uint8_t> valid_t;
  std::vector<double> rew_t, prg_t, prb_t;
  DevBuf d_dst, d_valid, d_rew, d_prg, d_prb;
  MdpDev M{};
};

static int mdp_upload(const cpr_mdp* mdp, MdpUpload& u, hipStream_t st) {
  const int64_t S = mdp->S, A = mdp->A, T = mdp->T, P = mdp->P;
  const int64_t AT = A * T, slots = AT * S;
  try {  // no exception may cross the C boundary
    u.dst_t.resize((size_t)slots);
    u.valid_t.resize((size_t)(A * S));
    u.rew_t.resize((size_t)slots);
    u.prg_t.resize((size_t)slots);
    u.prb_t.resize((size_t)(slots * P));
  } catch (const std::exception&) {
    return fail(CPR_E_CAPACITY, "mdp: out of host memory for the upload copies");
  }
  for (int64_t s = 0; s < S; ++s) {
    for (int64_t a = 0; a < A; ++a) u.valid_t[a * S + s] = mdp->valid[s * A + a] ? 1 : 0;
    for (int64_t j = 0; j < AT; ++j) {
      const int64_t from = s * AT + j, to = j * S + s;
      const bool use = mdp->used[from] != 0;  // the kernels load unused slots too: dst -1, zeros
      u.dst_t[to] = use ? mdp->dst[from] : -1;
      u.rew_t[to] = use ? mdp->rew[from] : 0.0;
      u.prg_t[to] = use ? mdp->prg[from] : 0.0;
      for (int64_t p = 0; p < P; ++p)
        u.prb_t[p * slots + to] = use ? mdp->prb[p * slots + from] : 0.0;
    }
  }
  HIP_TRY(u.d_dst.ensure((size_t)slots * 4));
  HIP_TRY(u.d_valid.ensure((size_t)(A * S)));
  HIP_TRY(u.d_rew.ensure((size_t)slots * 8));
  HIP_TRY(u.d_prg.ensure((size_t)slots * 8));
  HIP_TRY(u.d_prb.ensure((size_t)(slots * P) * 8));
  HIP_TRY(hipMemcpyAsync(u.d_dst.p, u.dst_t.data(), (size_t)slots * 4, hipMemcpyHostToDevice, st));
  HIP_TRY(hipMemcpyAsync(u.d_valid.p, u.valid_t.data(), (size_t)(A * S), hipMemcpyHostToDevice,
                         st));
  HIP_TRY(hipMemcpyAsync(u.d_rew.p, u.rew_t.data(), (size_t)slots * 8, hipMemcpyHostToDevice, st));
  HIP_TRY(hipMemcpyAsync(u.d_prg.p, u.prg_t.data(), (size_t)slots * 8, hipMemcpyHostToDevice, st));
  HIP_TRY(hipMemcpyAsync(u.d_prb.p, u.prb_t.data(), (size_t)(slots * P) * 8,
                         hipMemcpyHostToDevice, st));
  u.M = MdpDev{(int32_t)S, (int32_t)A, (int32_t)T, (int32_t)P, (const int32_t*)u.d_dst.p,
               (const uint8_t*)u.d_valid.p, (const double*)u.d_rew.p, (const double*)u.d_prg.p,
               (const double*)u.d_prb.p};
  return CPR_OK;
}

struct MdpEvents {
  hipEvent_t e0 = nullptr, e1 = nullptr;
  ~MdpEvents() {
    if (e0) (void)hipEventDestroy(e0);
    if (e1) (void)hipEventDestroy(e1);
  }
};

// The sweeps of either entry, between two events: every solve stops after `limit` sweeps at the
// latest, so both loops end: the resident one after limit / kMdpSweepsPerLaunch + 1 launches,
// the global one after launch limit + 1 (which records the stop of sweep `limit`). `status` is
// the host copy of the device's `d_status`, read between launches; `done`: none is running.
// (a template, so that each entry's launches are called directly: C++ linkage inside this block)
extern "C++" template <class LaunchResident, class LaunchSweep>
static int mdp_drive(bool resident, int64_t limit, std::vector<int32_t>& status,
                     const void* d_status, hipStream_t st, MdpEvents& ev,
                     const LaunchResident& launch_resident, const LaunchSweep& launch_sweep,
                     bool& done) {
  auto all_stopped = [&]() {
    for (int32_t v : status)
      if (v == kMdpRunning) return false;
    return true;
  };
  HIP_TRY(hipEventCreate(&ev.e0));
  HIP_TRY(hipEventCreate(&ev.e1));
  HIP_TRY(hipEventRecord(ev.e0, st));
  done = false;
  if (resident) {
    const int64_t launches = limit / kMdpSweepsPerLaunch + 1;
    for (int64_t l = 0; l < launches && !done; ++l) {
      HIP_TRY(launch_resident());
      HIP_TRY(hipMemcpyAsync(status.data(), d_status, status.size() * 4, hipMemcpyDeviceToHost,
                             st));
      HIP_TRY(hipStreamSynchronize(st));
      done = all_stopped();
    }
  } else {
    for (int64_t k = 1; k <= limit + 1 && !done;) {
      for (int n = 0; n < kMdpReadbackEvery && k <= limit + 1; ++n, ++k)
        HIP_TRY(launch_sweep(k));
      HIP_TRY(hipMemcpyAsync(status.data(), d_status, status.size() * 4, hipMemcpyDeviceToHost,
                             st));
      HIP_TRY(hipStreamSynchronize(st));
      done = all_stopped();
    }
  }
  HIP_TRY(hipEventRecord(ev.e1, st));
  return CPR_OK;
}

int cpr_mdp_value_iteration(cpr_ctx* ctx, const cpr_mdp* mdp, const cpr_mdp_vi_opts* opts,
                            cpr_mdp_vi_result* res) {
  if (!ctx || !mdp || !opts || !res) return fail(CPR_E_INVALID_ARG, "NULL argument");
  CPR_ENTER(ctx);
  // everything is checked before the first allocation or launch
  if (const int rc = mdp_check(mdp)) return rc;
  if (!res->value || !res->progress || !res->policy || !res->iter || !res->delta || !res->status)
    return fail(CPR_E_INVALID_ARG, "result: NULL array");
  if (!(opts->discount > 0.0 && opts->discount <= 1.0))
    return fail(CPR_E_INVALID_ARG, "discount must be in (0, 1]");
  if (!(opts->stop_delta >= 0.0)) return fail(CPR_E_INVALID_ARG, "stop_delta must be >= 0");
  if (opts->max_iter < 0) return fail(CPR_E_INVALID_ARG, "max_iter must be >= 0");
  if (opts->stop_delta == 0.0 && opts->max_iter == 0)
    return fail(CPR_E_INVALID_ARG, "infinite iteration: stop_delta == 0 and max_iter == 0");
  if (opts->path < CPR_MDP_VI_AUTO || opts->path > CPR_MDP_VI_GLOBAL)
    return fail(CPR_E_INVALID_ARG, "path: expected 0 (auto), 1 (resident) or 2 (global)");
  const int64_t S = mdp->S, A = mdp->A, T = mdp->T, P = mdp->P;
  const int64_t AT = A * T;
  HIP_TRY(hipSetDevice(ctx->device));
  const bool fits = mdp_resident_fits(S);
  if (opts->path == CPR_MDP_VI_RESIDENT && !fits)
    return fail(CPR_E_CAPACITY, "path resident: the states do not fit one workgroup's LDS");
  const bool resident =
      opts->path == CPR_MDP_VI_RESIDENT ||
      (opts->path == CPR_MDP_VI_AUTO && fits && mdp_auto_resident(AT * S, P, ctx->cus));
  const int64_t chunks = (S + kMdpBlock - 1) / kMdpBlock;
  if (!resident && chunks * P > INT32_MAX)
    return fail(CPR_E_CAPACITY, "path global: more than 2^31 workgroups per sweep");

  std::vector<int32_t> status;
  try {
    status.resize((size_t)P);
  } catch (const std::exception&) {
    return fail(CPR_E_CAPACITY, "mdp: out of host memory for the upload copies");
  }
  hipStream_t st = ctx->stream;
  MdpUpload up;
  if (const int rc = mdp_upload(mdp, up, st)) return rc;
  DevBuf d_val[2], d_pro[2], d_pol, d_status, d_iter, d_delta, d_acc;
  const size_t vec = (size_t)(P * S) * 8;
  for (int i = 0; i < (resident ? 1 : 2); ++i) {
    HIP_TRY(d_val[i].ensure(vec));
    HIP_TRY(d_pro[i].ensure(vec));
    HIP_TRY(hipMemsetAsync(d_val[i].p, 0, vec, ctx->stream));
    HIP_TRY(hipMemsetAsync(d_pro[i].p, 0, vec, ctx->stream));
  }
  HIP_TRY(d_pol.ensure((size_t)(P * S) * 4));
  HIP_TRY(d_status.ensure((size_t)P * 4));
  HIP_TRY(d_iter.ensure((size_t)P * 8));
  HIP_TRY(d_delta.ensure((size_t)P * 8));
  HIP_TRY(d_acc.ensure((size_t)P * 24));
  HIP_TRY(hipMemsetAsync(d_status.p, 0xFF, (size_t)P * 4, st));  // kMdpRunning
  HIP_TRY(hipMemsetAsync(d_iter.p, 0, (size_t)P * 8, st));
  HIP_TRY(hipMemsetAsync(d_delta.p, 0, (size_t)P * 8, st));
  HIP_TRY(hipMemsetAsync(d_acc.p, 0, (size_t)P * 24, st));

  const MdpDev& M = up.M;
  MdpRun R{};
  R.stop_delta = opts->stop_delta;
  R.discount = opts->discount;
  R.max_iter = opts->max_iter;
  R.cap = mdp_sweep_cap();
  for (int i = 0; i < 2; ++i) {
    R.value[i] = (double*)d_val[i].p;
    R.progress[i] = (double*)d_pro[i].p;
  }
  R.policy = (int32_t*)d_pol.p;
  R.status = (int32_t*)d_status.p;
  R.iter = (int64_t*)d_iter.p;
  R.delta = (double*)d_delta.p;
  R.acc = (unsigned long long*)d_acc.p;

  const int64_t limit = opts->max_iter > 0 ? opts->max_iter : R.cap;
  MdpEvents ev;
  bool done = false;
  if (const int rc = mdp_drive(
          resident, limit, status, d_status.p, st, ev,
          [&]() { return launch_mdp_resident(M, R, st); },
          [&](int64_t k) { return launch_mdp_sweep(M, R, k, st); }, done))
    return rc;
  if (!done) return fail(CPR_E_INTERNAL, "mdp value iteration: a point outlived its sweep limit");

  HIP_TRY(hipMemcpyAsync(res->iter, d_iter.p, (size_t)P * 8, hipMemcpyDeviceToHost, st));
  HIP_TRY(hipMemcpyAsync(res->delta, d_delta.p, (size_t)P * 8, hipMemcpyDeviceToHost, st));
  HIP_TRY(hipMemcpyAsync(res->policy, d_pol.p, (size_t)(P * S) * 4, hipMemcpyDeviceToHost, st));
  HIP_TRY(hipStreamSynchronize(st));
  if (resident) {
    HIP_TRY(hipMemcpyAsync(res->value, d_val[0].p, vec, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipMemcpyAsync(res->progress, d_pro[0].p, vec, hipMemcpyDeviceToHost, st));
  }
  for (int64_t p = 0; p < P && !resident; ++p) {
    // the global path left the point's vectors in the buffer its last sweep wrote
    const int i = (int)(res->iter[p] & 1);
    HIP_TRY(hipMemcpyAsync(res->value + p * S, (const double*)d_val[i].p + p * S, (size_t)S * 8,
                           hipMemcpyDeviceToHost, st));
    HIP_TRY(hipMemcpyAsync(res->progress + p * S, (const double*)d_pro[i].p + p * S,
                           (size_t)S * 8, hipMemcpyDeviceToHost, st));
  }
  HIP_TRY(hipStreamSynchronize(st));
  float ms = 0.f;
  HIP_TRY(hipEventElapsedTime(&ms, ev.e0, ev.e1));
  for (int64_t p = 0; p < P; ++p) res->status[p] = status[(size_t)p];
  res->path_used = resident ? CPR_MDP_VI_RESIDENT : CPR_MDP_VI_GLOBAL;
  res->kernel_ms = ms;
  return CPR_OK;
}

int cpr_mdp_pe_opts_default(cpr_mdp_pe_opts* opts) {
  if (!opts) return fail(CPR_E_INVALID_ARG, "opts is NULL");
  opts->theta = 1e-6;
  opts->discount = 1.0;
  opts->max_iter = 0;
  opts->path = CPR_MDP_VI_AUTO;
  return CPR_OK;
}

// as mdp_sweep_cap, for policy evaluation: CPR_MDP_PE_SWEEP_CAP lowers it
static int64_t mdp_pe_sweep_cap() {
  if (const char* e = getenv("CPR_MDP_PE_SWEEP_CAP")) {
    const long long v = atoll(e);
    if (v >= 1 && v < kMdpSweepCap) return v;
  }
  return kMdpSweepCap;
}

// explicit_mdp.py:179-208 for every evaluation, folded into the policy: act[e][s] = policy[e][s]
// where state s is included and has a policy entry, else -1 (the state stays 0)
static void mdp_pe_included(const cpr_mdp* mdp, const cpr_mdp_pe* job, std::vector<int32_t>& act,
                            std::vector<int32_t>& todo, std::vector<uint8_t>& seen) {
  const int64_t S = mdp->S, A = mdp->A, T = mdp->T, slots = A * T * S;
  for (int64_t e = 0; e < job->E; ++e) {
    const int32_t* pol = job->policy + e * S;
    int32_t* out = act.data() + e * S;
    if (job->states == CPR_MDP_PE_ALL) {
      for (int64_t s = 0; s < S; ++s) out[s] = pol[s] < 0 ? -1 : pol[s];
      continue;
    }
    const double* prb = mdp->prb + (int64_t)job->point[e] * slots;
    std::fill(seen.begin(), seen.end(), (uint8_t)0);
    todo.clear();
    for (int32_t i = 0; i < job->n_start; ++i) {
      const int32_t s = job->start_state[e * job->n_start + i];
      if (job->start_prob[e * job->n_start + i] > 0.0 && !seen[s]) {
        seen[s] = 1;
        todo.push_back(s);
      }
    }
    while (!todo.empty()) {
      const int32_t s = todo.back();
      todo.pop_back();
      if (pol[s] < 0) continue;  // a leaf
      const int64_t base = ((int64_t)s * A + pol[s]) * T;
      for (int64_t t = 0; t < T; ++t) {
        if (!mdp->used[base + t] || prb[base + t] == 0.0) continue;
        const int32_t d = mdp->dst[base + t];
        if (!seen[d]) {
          seen[d] = 1;
          todo.push_back(d);
        }
      }
    }
    for (int64_t s = 0; s < S; ++s) out[s] = seen[s] && pol[s] >= 0 ? pol[s] : -1;
  }
}

int cpr_mdp_policy_evaluation(cpr_ctx* ctx, const cpr_mdp* mdp, const cpr_mdp_pe* job,
                              const cpr_mdp_pe_opts* opts, cpr_mdp_pe_result* res) {
  if (!mdp || !job || !opts || !res) return fail(CPR_E_INVALID_ARG, "NULL argument");
  // everything is checked before the context is touched, an allocation made or a launch issued
  if (const int rc = mdp_check(mdp)) return rc;
  if (!res->reward || !res->progress || !res->iter || !res->delta || !res->status)
    return fail(CPR_E_INVALID_ARG, "result: NULL array");
  if (!(opts->discount > 0.0 && opts->discount <= 1.0))
    return fail(CPR_E_INVALID_ARG, "discount must be in (0, 1]");
  if (!(opts->theta >= 0.0)) return fail(CPR_E_INVALID_ARG, "theta must be >= 0");
  if (opts->max_iter < 0) return fail(CPR_E_INVALID_ARG, "max_iter must be >= 0");
  if (opts->theta == 0.0 && opts->max_iter == 0)
    return fail(CPR_E_INVALID_ARG, "infinite iteration: theta == 0 and max_iter == 0");
  if (opts->path < CPR_MDP_VI_AUTO || opts->path > CPR_MDP_VI_GLOBAL)
    return fail(CPR_E_INVALID_ARG, "path: expected 0 (auto), 1 (resident) or 2 (global)");
  const int64_t S = mdp->S, A = mdp->A, T = mdp->T, P = mdp->P, E = job->E;
  if (E < 1) return fail(CPR_E_INVALID_ARG, "job: E must be at least 1");
  if (E > ((int64_t)1 << 36) / S)
    return fail(CPR_E_INVALID_ARG, "job: more than 2^36 states over all evaluations");
  if (!job->point || !job->policy) return fail(CPR_E_INVALID_ARG, "job: NULL array");
  if (job->states != CPR_MDP_PE_REACHABLE && job->states != CPR_MDP_PE_ALL)
    return fail(CPR_E_INVALID_ARG, "job: states: expected 0 (reachable) or 1 (all)");
  for (int64_t e = 0; e < E; ++e)
    if (job->point[e] < 0 || job->point[e] >= P)
      return fail(CPR_E_INVALID_ARG, "job: a point is outside [0, P)");
  for (int64_t i = 0; i < E * S; ++i) {
    const int32_t a = job->policy[i];
    if (a >= A || (a >= 0 && !mdp->valid[(i % S) * A + a]))
      return fail(CPR_E_INVALID_ARG, "job: a policy entry names an action its state does not offer");
  }
  if (job->states == CPR_MDP_PE_REACHABLE) {
    if (job->n_start < 1) return fail(CPR_E_INVALID_ARG, "job: n_start must be at least 1");
    if (!job->start_state || !job->start_prob)
      return fail(CPR_E_INVALID_ARG, "job: NULL start array");
    if (E > ((int64_t)1 << 36) / job->n_start)
      return fail(CPR_E_INVALID_ARG, "job: more than 2^36 start entries over all evaluations");
    for (int64_t i = 0; i < E * job->n_start; ++i)
      if (job->start_state[i] < 0 || job->start_state[i] >= S)
        return fail(CPR_E_INVALID_ARG, "job: a start state is outside [0, S)");
  }
  if (!ctx) return fail(CPR_E_INVALID_ARG, "ctx is NULL");
  CPR_ENTER(ctx);
  HIP_TRY(hipSetDevice(ctx->device));
  const bool fits = mdp_pe_resident_fits(S);
  if (opts->path == CPR_MDP_VI_RESIDENT && !fits)
    return fail(CPR_E_CAPACITY, "path resident: the states do not fit one workgroup's LDS");
  const char* reread_env = getenv("CPR_MDP_PE_REREAD");  // measurements: never keep the slots
  const bool reread = reread_env && atoi(reread_env) != 0;
  const bool keep = !reread && mdp_pe_resident_keeps(S, (int32_t)T);
  const bool resident =
      opts->path == CPR_MDP_VI_RESIDENT ||
      (opts->path == CPR_MDP_VI_AUTO && fits && mdp_pe_auto_resident(T * S, E, ctx->cus, keep));
  const int64_t chunks = (S + kMdpBlock - 1) / kMdpBlock;
  if (E > INT32_MAX || (!resident && chunks * E > INT32_MAX))
    return fail(CPR_E_CAPACITY, "more than 2^31 workgroups per sweep");

  std::vector<int32_t> status, act, todo;
  std::vector<uint8_t> seen;
  try {
    status.resize((size_t)E);
    act.resize((size_t)(E * S));
    todo.reserve((size_t)S);
    seen.resize((size_t)S);
  } catch (const std::exception&) {
    return fail(CPR_E_CAPACITY, "mdp: out of host memory for the upload copies");
  }
  mdp_pe_included(mdp, job, act, todo, seen);

  hipStream_t st = ctx->stream;
  MdpUpload up;
  if (const int rc = mdp_upload(mdp, up, st)) return rc;
  DevBuf d_rew[2], d_pro[2], d_act, d_point, d_status, d_iter, d_delta, d_acc;
  const size_t vec = (size_t)(E * S) * 8;
  for (int i = 0; i < (resident ? 1 : 2); ++i) {
    HIP_TRY(d_rew[i].ensure(vec));
    HIP_TRY(d_pro[i].ensure(vec));
    HIP_TRY(hipMemsetAsync(d_rew[i].p, 0, vec, st));
    HIP_TRY(hipMemsetAsync(d_pro[i].p, 0, vec, st));
  }
  HIP_TRY(d_act.ensure((size_t)(E * S) * 4));
  HIP_TRY(d_point.ensure((size_t)E * 4));
  HIP_TRY(d_status.ensure((size_t)E * 4));
  HIP_TRY(d_iter.ensure((size_t)E * 8));
  HIP_TRY(d_delta.ensure((size_t)E * 8));
  HIP_TRY(d_acc.ensure((size_t)E * 24));
  HIP_TRY(hipMemcpyAsync(d_act.p, act.data(), (size_t)(E * S) * 4, hipMemcpyHostToDevice, st));
  HIP_TRY(hipMemcpyAsync(d_point.p, job->point, (size_t)E * 4, hipMemcpyHostToDevice, st));
  HIP_TRY(hipMemsetAsync(d_status.p, 0xFF, (size_t)E * 4, st));  // kMdpRunning
  HIP_TRY(hipMemsetAsync(d_iter.p, 0, (size_t)E * 8, st));
  HIP_TRY(hipMemsetAsync(d_delta.p, 0, (size_t)E * 8, st));
  HIP_TRY(hipMemsetAsync(d_acc.p, 0, (size_t)E * 24, st));

  const MdpDev& M = up.M;
  MdpPeRun R{};
  R.theta = opts->theta;
  R.discount = opts->discount;
  R.max_iter = opts->max_iter;
  R.cap = mdp_pe_sweep_cap();
  R.E = (int32_t)E;
  R.reread = reread ? 1 : 0;
  R.point = (const int32_t*)d_point.p;
  R.act = (const int32_t*)d_act.p;
  for (int i = 0; i < 2; ++i) {
    R.reward[i] = (double*)d_rew[i].p;
    R.progress[i] = (double*)d_pro[i].p;
  }
  R.status = (int32_t*)d_status.p;
  R.iter = (int64_t*)d_iter.p;
  R.delta = (double*)d_delta.p;
  R.acc = (unsigned long long*)d_acc.p;

  const int64_t limit = opts->max_iter > 0 ? opts->max_iter : R.cap;
  MdpEvents ev;
  bool done = false;
  if (const int rc = mdp_drive(
          resident, limit, status, d_status.p, st, ev,
          [&]() { return launch_mdp_pe_resident(M, R, st); },
          [&](int64_t k) { return launch_mdp_pe_sweep(M, R, k, st); }, done))
    return rc;
  if (!done)
    return fail(CPR_E_INTERNAL, "mdp policy evaluation: an evaluation outlived its sweep limit");

  HIP_TRY(hipMemcpyAsync(res->iter, d_iter.p, (size_t)E * 8, hipMemcpyDeviceToHost, st));
  HIP_TRY(hipMemcpyAsync(res->delta, d_delta.p, (size_t)E * 8, hipMemcpyDeviceToHost, st));
  if (resident) {
    HIP_TRY(hipMemcpyAsync(res->reward, d_rew[0].p, vec, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipMemcpyAsync(res->progress, d_pro[0].p, vec, hipMemcpyDeviceToHost, st));
  } else {
    // the global path left an evaluation's vectors in the buffer its last sweep wrote: both
    // buffers come down whole and each evaluation's rows are taken from its own
    std::vector<double> other;
    try {
      other.resize((size_t)(E * S) * 2);
    } catch (const std::exception&) {
      return fail(CPR_E_CAPACITY, "mdp: out of host memory for the result copies");
    }
    HIP_TRY(hipMemcpyAsync(res->reward, d_rew[0].p, vec, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipMemcpyAsync(res->progress, d_pro[0].p, vec, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipMemcpyAsync(other.data(), d_rew[1].p, vec, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipMemcpyAsync(other.data() + E * S, d_pro[1].p, vec, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    for (int64_t e = 0; e < E; ++e) {
      if (!(res->iter[e] & 1)) continue;
      std::copy_n(other.data() + e * S, S, res->reward + e * S);
      std::copy_n(other.data() + E * S + e * S, S, res->progress + e * S);
    }
  }
  HIP_TRY(hipStreamSynchronize(st));
  float ms = 0.f;
  HIP_TRY(hipEventElapsedTime(&ms, ev.e0, ev.e1));
  for (int64_t e = 0; e < E; ++e) res->status[e] = status[(size_t)e];
  res->path_used = resident ? CPR_MDP_VI_RESIDENT : CPR_MDP_VI_GLOBAL;
  res->kernel_ms = ms;
  return CPR_OK;
}

}  // extern "C"
