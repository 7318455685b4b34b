/*
 * libcpr_hip — MI355X-native batched episode engine for pkel/cpr's gym hot path.
 *
 * C ABI (plain pointers and sizes, no exceptions across the boundary). Every entry
 * point returns an int status (CPR_OK = 0, negative = error); cpr_last_error() holds a
 * message for the calling thread.
 *
 * Reference interfaces each group of entry points replaces (file:line under the
 * pkel/cpr tree):
 *   cpr_version                    -> engine.cpr_lib_version   simulator/gym/cpr_gym_engine.ml:41
 *   cpr_batch_create               -> engine.create + Engine.Parameters.t + Engine.of_module
 *                                      simulator/gym/cpr_gym_engine.ml:42-89,
 *                                      simulator/gym/engine.ml:37-51,97-107
 *   cpr_reset                      -> engine.reset             cpr_gym_engine.ml:90-95, engine.ml:164-170
 *   cpr_step                       -> engine.step              cpr_gym_engine.ml:96-109, engine.ml:176-249
 *   cpr_policy_actions             -> engine.policies(...)[name](obs)
 *                                                              cpr_gym_engine.ml:110-138, engine.ml:258-261
 *   cpr_observation_spec           -> engine.n_actions / observation_low / observation_high
 *                                                              cpr_gym_engine.ml:146-162
 *   cpr_policy_name                -> keys of engine.policies  nakamoto_ssz.ml:342-350
 *   cpr_run_episodes               -> a Python loop of env.reset()/env.step(env.policy(obs))
 *                                      (experiments/rl-eval, gym/ocaml/test/test_benchmark.py:5-15)
 *                                      fused into one device launch per batch
 *   cpr_run_episodes (LOOP mode)   -> Simulator.loop ~activations + head
 *                                      simulator/lib/simulator.ml:519-543, csv_runner.ml:56-98
 *   cpr_node_outputs               -> the per-node `activations` / `reward` columns of a
 *                                      csv_runner.ml:74-79 row (Simulator state.activations,
 *                                      (Dag.data head).rewards, simulator.ml:377-388)
 *   cpr_stream_fill                -> the randomness the reference draws from OCaml Random
 *                                      (distributions.ml:17,24,90,93; simulator.ml:123),
 *                                      re-specified as a keyed Philox stream
 */
#ifndef CPR_HIP_H
#define CPR_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define CPR_ABI_VERSION 11

typedef struct cpr_ctx cpr_ctx;
typedef struct cpr_batch cpr_batch;

enum cpr_status {
  CPR_OK = 0,
  CPR_E_INVALID_ARG = -1,   /* engine.ml:37-51 Failure / network.ml:63-72 Invalid_argument */
  CPR_E_UNSUPPORTED = -2,   /* configuration the device engine does not implement */
  CPR_E_HIP = -3,           /* HIP runtime error */
  CPR_E_CAPACITY = -4,      /* lane capacity exceeded */
  CPR_E_STATE = -5,         /* call order violated (step before reset, ...) */
  CPR_E_INTERNAL = -6       /* the library contradicted one of its own invariants */
};

enum cpr_protocol {
  CPR_PROTO_NAKAMOTO = 0, /* nakamoto.ml + nakamoto_ssz.ml */
  CPR_PROTO_ETHEREUM = 1, /* ethereum.ml Byzantium + ethereum_ssz.ml (cpr_protocols.ml:39-49) */
  CPR_PROTO_BK = 2,       /* bk.ml + bk_ssz.ml (cpr_protocols.ml:53-72), k = cpr_config.k */
  CPR_PROTO_TAILSTORM = 3, /* tailstorm.ml + tailstorm_ssz.ml (cpr_protocols.ml:153-175),
                             k = cpr_config.k, selection = cpr_config.subblock_selection */
  CPR_PROTO_FC16 = 4,      /* the FC'16 abstract selfish-mining model with probabilistic
                             termination, gym/rust/src/fc16.rs FC16SSZwPT: alpha, gamma,
                             horizon, policy = enum cpr_fc16_policy; fused episodes only
                             (cpr_run_episodes); max_steps caps an episode (CPR_ST_CAPACITY) */
  CPR_PROTO_FC16_ENV = 5,  /* the same model as a lockstep env (additive within ABI v11; a new
                             id because CPR_PROTO_FC16 keeps refusing every lockstep entry).
                             cpr_run_episodes as CPR_PROTO_FC16, and with n_lanes > 0:
                             cpr_reset / cpr_step (action = index 0..3 into the offered list
                             [Wait, Adopt, Override if a > h, Match if a >= h], an index beyond
                             the list acts as Wait, fc16.rs:49-60,182; observation x / (1 + x)
                             of (a, h, fork), unit_observation ignored; done = terminated, or
                             max_steps steps: CPR_ST_CAPACITY), cpr_observe_fields (a, h, fork),
                             the policy network, cpr_rollout_net(_env), the lane env, the
                             learner, Q-learning (cpr_dqn_*) and cpr_eval_net.
                             CPR_E_UNSUPPORTED: cpr_rollout,
                             cpr_policy_actions, cpr_replay, cpr_node_outputs and
                             CPR_GYM_REWARD_DENSE_PER_PROGRESS (no progress target) */
  CPR_PROTO_GENERIC_NAKAMOTO = 6 /* the reference's generic release/consider env over Nakamoto,
                             gym/rust/src/generic/mod.rs with proto/nakamoto.rs (Nakamoto-v0), as
                             lockstep lanes over a per-lane block DAG (additive within ABI v11;
                             generic_lane.h). alpha, gamma, horizon as FC16;
                             max_steps is required (1 .. 4096: a lane holds max_steps + 1
                             blocks; CPR_E_INVALID_ARG otherwise) and truncates with
                             CPR_ST_CAPACITY; k in 1..11 sizes the network's action head.
                             cpr_step takes the reference's integers (mod.rs:214-220): 0
                             Continue, -(i+1) Release(i), +(i+1) Consider(i), clamped to +-256;
                             an index past its list acts as the list's last entry, an empty
                             list as Continue. Network entries (cpr_rollout_net(_env),
                             cpr_eval_net, cpr_dqn_*, the learner's buffers) use a head of
                             1 + 2k actions: 0 Continue, 1..k Release(0..k-1), k+1..2k
                             Consider(0..k-1). Observation: the reference's five f32 widened to
                             double (a - ca, d - ca, match feasible, encoded last release,
                             encoded last consider); unit_observation ignored. Reward: the
                             step's attacker reward on the defenders' chain. Step infos: episode
                             sums, n_activations = blocks mined + 1, head_height = the
                             defenders' entry, head_miner -1. cpr_observe_fields: seven int32
                             (a, d, match feasible, n_release, n_consider, n_blocks, the last
                             step's rewrites). A lane whose episode is over ignores steps until
                             its reset. CPR_E_UNSUPPORTED: cpr_run_episodes, cpr_rollout,
                             cpr_policy_actions, cpr_replay, cpr_node_outputs,
                             CPR_GYM_REWARD_DENSE_PER_PROGRESS and CPR_FC16_ROLLOUT_FUSED */
};

/* policies of the FC16 model (fc16_lane.h); a table maps (a, h, fork) to an action name
 * CPR_FC16_WAIT .. CPR_FC16_MATCH: table[(min(a,D-1)*D + min(h,D-1))*3 + fork],
 * fork 0 irrelevant, 1 relevant, 2 active (fc16.rs:7-11) */
enum cpr_fc16_policy { CPR_FC16_POLICY_HONEST = 0, CPR_FC16_POLICY_SM1 = 1, CPR_FC16_POLICY_TABLE = 2 };
enum cpr_fc16_action { CPR_FC16_WAIT = 0, CPR_FC16_ADOPT = 1, CPR_FC16_OVERRIDE = 2, CPR_FC16_MATCH = 3 };

/* incentive schemes (ethereum.ml:3,173-197; bk.ml:3,151-176) */
enum cpr_reward_scheme {
  CPR_REWARD_CONSTANT = 0, /* Ethereum `Constant` (whitepaper): uncle 15/16;
                              B_k `Constant`: 1 per confirmed vote to its miner */
  CPR_REWARD_DISCOUNT = 1, /* Ethereum `Discount` (Byzantium): uncle (8 - dh) / 8 */
  CPR_REWARD_BLOCK = 2,    /* B_k `Block`: k to the block's signer (leader) */
  CPR_REWARD_PUNISH = 3,   /* Tailstorm `Punish`: 1 per vote on the longest vote branch */
  CPR_REWARD_HYBRID = 4    /* Tailstorm `Hybrid`: depth/k per vote on the longest branch;
                              Tailstorm also takes CONSTANT (1 per vote) and DISCOUNT (depth/k
                              per confirmed vote), tailstorm.ml:3,204-227 */
};

/* Tailstorm sub-block (quorum) selection, tailstorm.ml:4,262-507 */
enum cpr_subblock_selection {
  CPR_SELECT_ALTRUISTIC = 0,
  CPR_SELECT_HEURISTIC = 1,
  CPR_SELECT_OPTIMAL = 2 /* brute force over n-choose-k <= 100, else heuristic */
};

/* policy ids of the tailstorm_ssz attack space (tailstorm_ssz.ml:365-472) */
enum cpr_tailstorm_policy {
  CPR_TS_POLICY_HONEST = 0,
  CPR_TS_POLICY_GET_AHEAD = 1,
  CPR_TS_POLICY_MINOR_DELAY = 2,
  CPR_TS_POLICY_AVOID_LOSS = 3,   /* avoid_loss_alt, registered as "avoid-loss" */
  CPR_TS_POLICY_AVOID_LOSS_A = 4, /* avoid_loss */
  CPR_TS_POLICY_AVOID_LOSS_B = 5, /* avoid_loss_alt2 */
  CPR_TS_POLICY_LONG_DELAY = 6,
  CPR_TS_POLICY_TABLE = 7, /* Action8 = table[((((min(pub,D-1)*D + min(priv,D-1))*(k+1)
                             + min(public_votes,k))*(k+1) + min(private_votes_inclusive,k))*3
                             + event] with D = policy_table_dim (the B_k layout) */
  CPR_TS_POLICY_RANDOM = 8 /* loop tasks: a keyed random Action8 at every decision (the
                              reference's random attacker, cpr_protocols.ml:658-782) */
};

/* policy ids of the bk_ssz attack space (bk_ssz.ml:346-415; "avoid-loss" is avoid_loss_alt) */
enum cpr_bk_policy {
  CPR_BK_POLICY_HONEST = 0,
  CPR_BK_POLICY_GET_AHEAD = 1,
  CPR_BK_POLICY_MINOR_DELAY = 2,
  CPR_BK_POLICY_AVOID_LOSS = 3,
  CPR_BK_POLICY_TABLE = 4, /* action = table[((((min(pub,D-1)*D + min(priv,D-1))*(k+1)
                             + min(public_votes,k))*(k+1) + min(private_votes_inclusive,k))*3
                             + event] with D = policy_table_dim */
  CPR_BK_POLICY_RANDOM = 5 /* loop tasks: a keyed random Action8 at every decision
                              (cpr_protocols.ml:658-782) */
};

/* ssz_tools.ml:230-263 Action8, Variants.to_rank */
enum cpr_action8 {
  CPR_ADOPT_PROLONG = 0, CPR_OVERRIDE_PROLONG = 1, CPR_MATCH_PROLONG = 2, CPR_WAIT_PROLONG = 3,
  CPR_ADOPT_PROCEED = 4, CPR_OVERRIDE_PROCEED = 5, CPR_MATCH_PROCEED = 6, CPR_WAIT_PROCEED = 7
};

/* policy ids of the ethereum_ssz attack space (ethereum_ssz.ml:444-538) */
enum cpr_ethereum_policy {
  CPR_ETH_POLICY_HONEST = 0,
  CPR_ETH_POLICY_SELFISH_RELEASE = 1,
  CPR_ETH_POLICY_SELFISH_DISCARD = 2,
  CPR_ETH_POLICY_FN19 = 3,
  CPR_ETH_POLICY_FN19PKEL = 4,
  CPR_ETH_POLICY_TABLE = 5, /* action (0..23) = table[(min(public_height,D-1)*D
                              + min(private_height,D-1))*2 + event], D = policy_table_dim */
  CPR_ETH_POLICY_RANDOM = 6 /* loop tasks: a keyed random action of 24 at every decision
                               (cpr_protocols.ml:658-782) */
};

/* ethereum_ssz.ml:161-277: action = rank * 4 + own * 2 + foreign, rank in
 * {Adopt_discard, Adopt_release, Override, Match, Release1, Wait} */
enum cpr_ethereum_action_rank {
  CPR_ETH_ADOPT_DISCARD = 0, CPR_ETH_ADOPT_RELEASE = 1, CPR_ETH_OVERRIDE = 2,
  CPR_ETH_MATCH = 3, CPR_ETH_RELEASE1 = 4, CPR_ETH_WAIT = 5
};

enum cpr_network {
  CPR_NET_SELFISH_MINING = 0, /* network.ml:61-105, as the gym builds it (engine.ml:100-107) */
  CPR_NET_TWO_AGENTS = 1,     /* network.ml:50-59 */
  CPR_NET_HONEST_CLIQUE = 2,  /* experiments/simulate/models.ml:3-28 honest_clique: `defenders`
                                 = n honest nodes (2..64), node i has compute i + 1, every
                                 link delay uniform [delay_lo, delay_hi), simple
                                 dissemination; CPR_MODE_LOOP, Nakamoto or Ethereum */
  CPR_NET_EXP_CLIQUE = 3,     /* Network.T.symmetric_clique with exponential propagation
                                 (cpr_protocols.ml:200-210,478-485): node 0 (the attacker,
                                 running cfg.policy) plus `defenders` honest nodes (1..63),
                                 equal compute, every link delay exponential with mean
                                 propagation_delay; CPR_MODE_LOOP, every protocol
                                 (Nakamoto on the exact event engine in Nakamoto mode) */
  CPR_NET_ABSTRACT_GAMMA = 4  /* FLAGGED abstract-gamma mode (not a network
                                 of the reference, which rejects gamma = 1, envs.py:73-75):
                                 the gym's attacker + `defenders` equal-compute honest nodes
                                 with zero propagation delays, where a release that ties the
                                 window's fresh defender block wins at each defender, its
                                 miner included, iff that defender's coin
                                 U(k, 0, j) < gamma (Eyal-Sirer'14 gamma, exact for any
                                 gamma in [0, 1]); every other tie keeps the first-received
                                 block. Nakamoto, CPR_MODE_GYM; no replay, no node outputs */
};

enum cpr_mode {
  CPR_MODE_GYM = 0,  /* episode = reset + steps until done (engine.ml:209-214) */
  CPR_MODE_LOOP = 1  /* episode = Simulator.loop ~activations (simulator.ml:519-533) */
};

/* policy ids of the nakamoto_ssz attack space, nakamoto_ssz.ml:274-350 */
enum cpr_policy {
  CPR_POLICY_HONEST = 0,
  CPR_POLICY_SIMPLE = 1,
  CPR_POLICY_EYAL_SIRER_2014 = 2,
  CPR_POLICY_SAPIRSHTEIN_2016_SM1 = 3,
  CPR_POLICY_TABLE = 4, /* action = table[(min(pub,D-1)*D + min(priv,D-1))*2 + event] */
  CPR_POLICY_RANDOM = 5 /* loop tasks on the event engine (cpr_protocols.ml:658-782): a keyed
                           random action of 4 at every decision; the i-th decision of an
                           episode draws word 0 of Philox block (i, 0x50000000) and takes
                           (w0 * n) >> 32 (every protocol's *_POLICY_RANDOM likewise) */
};

/* nakamoto_ssz.ml:116-154, Variants.to_rank */
enum cpr_nakamoto_action { CPR_ADOPT = 0, CPR_OVERRIDE = 1, CPR_MATCH = 2, CPR_WAIT = 3 };

/* per-episode status bits */
enum cpr_episode_status {
  CPR_ST_OK = 0u,
  CPR_ST_TIE = 1u,      /* a defender resolved an equal-time, equal-height delivery */
  CPR_ST_OVERLAP = 2u,  /* Nakamoto: an activation fired while finite-delay messages were in
                           flight; the episode is re-run exactly (CPR_ST_EXACT_RERUN) */
  CPR_ST_DEEP_FORK = 4u,      /* Nakamoto: private chain beyond its slots */
  CPR_ST_TIE_UNRESOLVED = 8u, /* Nakamoto: tie replay capacity exceeded */
  CPR_ST_STALE_TIME = 16u,    /* Nakamoto: head time older than the time log */
  CPR_ST_CAPACITY = 32u,      /* event-engine lanes (Ethereum, B_k, Tailstorm): a lane
                                 capacity (vertex ring, event heap, candidate lists, frontier,
                                 Tailstorm brute-force budget) was exceeded; the episode's
                                 outputs are not valid */
  CPR_ST_REFERENCE_RAISES = 64u, /* Tailstorm: the reference raises an exception at this point
                                 (List.for_all2 in summary dedup, Division_by_zero in
                                 n_choose_k, assert false in heuristic_quorum); the episode
                                 stops, outputs not valid */
  CPR_ST_TRACE_MISS = 128u,     /* cpr_replay: the episode needed a draw its trace does not
                                 hold (too few activations, a missing delay key); outputs
                                 not valid */
  CPR_ST_EXACT_RERUN = 256u     /* Nakamoto fused episodes (cpr_run_episodes, cpr_replay) and
                                 lockstep lanes (cpr_step): the closed-form lane flagged the
                                 episode (OVERLAP, DEEP_FORK, TIE_UNRESOLVED, STALE_TIME) and it
                                 was simulated again on the exact event engine (DESIGN.md
                                 §4.3); its outputs are that re-run's, and the lane's flags
                                 are kept beside this bit */
};

/* status bits that make an episode's outputs invalid; such episodes never enter a
 * summary's sums (cpr_summary.invalid counts them). A Nakamoto lockstep lane (cpr_step)
 * whose step sets OVERLAP, DEEP_FORK, TIE_UNRESOLVED or STALE_TIME is simulated again on the
 * exact event engine from its first draw and the actions it was given, and stays there
 * until its next reset: its outputs are exact and its status carries CPR_ST_EXACT_RERUN
 * beside those bits. Only a lane that cannot move (all exact slots of the batch in use, an
 * episode longer than its action log, a network the exact engine does not hold) reports
 * the bits without CPR_ST_EXACT_RERUN, and its outputs are then not exact. */
#define CPR_ST_INVALID (CPR_ST_CAPACITY | CPR_ST_REFERENCE_RAISES | CPR_ST_TRACE_MISS)
#define CPR_ST_LOCKSTEP_INEXACT \
  (CPR_ST_OVERLAP | CPR_ST_DEEP_FORK | CPR_ST_TIE_UNRESOLVED | CPR_ST_STALE_TIME)

typedef struct cpr_config {
  int32_t protocol;          /* enum cpr_protocol */
  int32_t network;           /* enum cpr_network */
  int32_t mode;              /* enum cpr_mode */
  int32_t policy;            /* enum cpr_policy; for cpr_step lanes the caller acts */
  const uint8_t* policy_table; /* host pointer: the *_POLICY_TABLE of the protocol */
  int32_t policy_table_dim;
  int32_t unit_observation;  /* ssz_tools.ml NormalizeObs ~unit */
  double alpha;              /* attacker compute, [0,1] */
  double gamma;              /* selfish-mining gamma, [0,1] */
  int32_t defenders;         /* >= 2 for CPR_NET_SELFISH_MINING */
  int32_t reward_scheme;     /* enum cpr_reward_scheme (Ethereum) */
  double activation_delay;   /* expected block interval, > 0 */
  double propagation_delay;  /* defender<->defender delay; the gym uses 1e-9 */
  int64_t max_steps;         /* GYM mode termination; <= 0 means max_int */
  double max_progress;       /* GYM mode termination; <= 0 means +inf */
  double max_time;           /* GYM mode termination; <= 0 means +inf */
  int64_t activations;       /* LOOP mode: activations per episode */
  uint64_t seed;             /* keyed-stream seed */
  int64_t n_lanes;           /* lockstep lanes for cpr_reset/cpr_step; 0 = none */
  int32_t k;                 /* B_k / Tailstorm: votes per block (bk.ml:7), >= 1 */
  int32_t subblock_selection;/* Tailstorm: enum cpr_subblock_selection */
  double delay_lo, delay_hi;  /* CPR_NET_HONEST_CLIQUE link delays U[lo, hi); NaN, NaN = the
                                 models.ml default 0.5, 1.5 (0, 0 is a real zero delay) */
  double horizon;             /* CPR_PROTO_FC16: expected progress before termination, >= 1 */
} cpr_config;

/* one finished episode; identical layout is produced by the CPU oracle */
typedef struct cpr_episode_record {
  double reward_attacker;    /* head.rewards[0]              engine.ml:215-219 */
  double reward_defender;    /* sum of head.rewards[1..]     */
  double progress;           /* Ref.progress head            engine.ml:208 */
  double chain_time;         /* Simulator.timestamp head     simulator.ml:14-21 */
  double sim_time;           /* clock.now                    */
  int64_t n_steps;           /* episode_n_steps              engine.ml:236 */
  int64_t n_activations;     /* episode_n_activations        engine.ml:237 */
  int32_t head_height;
  int32_t head_miner;        /* -1 = n/a (genesis); B_k: the head block's signer (leader) */
  uint32_t status;           /* enum cpr_episode_status bits */
  int32_t head_work;         /* Ethereum head work (ethereum.ml:93-97); 0 for Nakamoto */
} cpr_episode_record;

#define CPR_HIST_BINS 64

/* batch reduction; integer-exact so 1/2/4/8-GPU totals are bit-identical */
typedef struct cpr_summary {
  int64_t episodes;
  int64_t steps;
  int64_t activations;
  int64_t reward_attacker_fx;   /* sum of reward_attacker * 2^20 */
  int64_t reward_defender_fx;   /* sum of reward_defender * 2^20 */
  int64_t progress_fx;          /* sum of progress * 2^20 */
  uint64_t rel_revenue_fx;      /* sum of round(attacker/(attacker+defender) * 2^32) */
  uint64_t rel_revenue_sq_fx;   /* sum of round((attacker/(attacker+defender))^2 * 2^32) */
  int64_t orphans;              /* activations - head height */
  /* status_tie / status_overlap are diagnostics of the route that ran: the closed-form
     Nakamoto lane and the Ethereum window lane set CPR_ST_TIE when they replay a
     same-instant race and CPR_ST_OVERLAP when they hand an episode to the exact re-run;
     the per-lane event engines follow the reference's queue and set neither. Every other
     field is route-independent. */
  int64_t status_tie;           /* episodes with CPR_ST_TIE */
  int64_t status_overlap;       /* episodes with CPR_ST_OVERLAP */
  int64_t status_other;         /* valid episodes with other status bits */
  int64_t hist[CPR_HIST_BINS];  /* relative revenue histogram, bin = floor(rel*64) */
  int64_t invalid;              /* episodes with CPR_ST_INVALID bits: counted here and in
                                   steps / activations only, never in episodes or any sum */
} cpr_summary;

/* lockstep info, structure of arrays, one entry per lane (engine.ml:224-241) */
typedef struct cpr_step_info {
  double* episode_reward_attacker;
  double* episode_reward_defender;
  double* episode_progress;
  double* episode_chain_time;
  double* episode_sim_time;
  int64_t* episode_n_steps;
  int64_t* episode_n_activations;
  int32_t* head_height;
  int32_t* head_miner;
  uint32_t* status;  /* cpr_episode_status bits of the lane's episode (CPR_ST_INVALID: the
                        reference would have raised / the lane's capacity was exceeded;
                        CPR_ST_LOCKSTEP_INEXACT without CPR_ST_EXACT_RERUN: Nakamoto
                        outputs not exact) */
} cpr_step_info;

/* An exported activation/delay trace: every random draw of n_episodes
 * episodes, addressed by the coordinates of the keyed stream, so an episode replays
 * bit-exactly on any engine that consumes the same draws. Arrays are CSR over episodes
 * (x_offset has n_episodes + 1 entries, x_offset[0] = 0); all host pointers.
 *   act_miner[j], act_delay[j]  activation j's miner (the alias sample over compute shares,
 *                               distributions.ml:45-98 via simulator.ml:465-472) and the
 *                               exponential delay drawn when clock j is scheduled
 *                               (simulator.ml:170-173; j = 0 is the first clock)
 *   pow_hash[s]                 30-bit Random.bits of vertex serial s (simulator.ml:123);
 *                               B_k and Tailstorm only (may be empty otherwise)
 *   link_key[i], link_delay[i]  message delays drawn at Network Tx (simulator.ml:481-487),
 *                               keys ascending per episode:
 *                               Nakamoto, Ethereum: (kw << 32) | (off << 12) | dest with
 *                                 kw = activations when the share happened, off = the
 *                                 message's position in that share's order
 *                               B_k, Tailstorm: (serial << 32) | dest
 * Traces come from the CPU oracle (tests/oracle_py.py export_traces; with the OCaml 4.12
 * Random replica it records the reference's own stream) or from an instrumented OCaml
 * Simulator. */
typedef struct cpr_trace {
  int64_t n_episodes;
  const int64_t* act_offset;
  const int32_t* act_miner;
  const double* act_delay;
  const int64_t* pow_offset;
  const int32_t* pow_hash;
  const int64_t* link_offset;
  const uint64_t* link_key;
  const double* link_delay;
} cpr_trace;

const char* cpr_version(void);
int cpr_abi_version(void);
const char* cpr_last_error(void);

/* device_ordinal: HIP device index (one context per GPU / per process) */
int cpr_ctx_create(int device_ordinal, cpr_ctx** out);
int cpr_ctx_destroy(cpr_ctx* ctx);
int cpr_device_count(int* out);

int cpr_batch_create(cpr_ctx* ctx, const cpr_config* cfg, cpr_batch** out);
int cpr_batch_destroy(cpr_batch* b);

/* Run episodes [first_episode, first_episode + n_episodes) to completion on the device.
 * summary: host pointer, accumulated (+=) — zero it before the first call.
 * records: NULL, or n_episodes records; records_on_device != 0 means a device pointer.
 * Synchronous. */
int cpr_run_episodes(cpr_batch* b, int64_t n_episodes, uint64_t first_episode,
                     cpr_summary* summary, cpr_episode_record* records,
                     int records_on_device);
/* Same, asynchronous on the context's streams; summary must be a device pointer to a
 * zeroed cpr_summary and records (optional) a device pointer. Both are complete after
 * cpr_synchronize (Nakamoto: exact re-runs of flagged episodes, CPR_ST_EXACT_RERUN, run on
 * the context's stream at the next flush). Blocking point: a flush (cpr_synchronize, or one
 * forced inside this call when the context's re-run table or overflow-flag chunks are full)
 * waits for the stream to read how many episodes were queued, so that it can size the
 * re-run grid; an _async call that forces one therefore returns only after the launches
 * before it have finished.
 * The launch itself may be deferred until then. Nakamoto summary-only calls (no records)
 * on the gym's selfish-mining network with two defenders (gamma = 0, or 0 < gamma <= .5), a
 * built-in policy and only max_steps <= 2^14 ending the episode wait in the context's pending
 * group; calls that share seed, first_episode, n_episodes and every parameter but alpha (a
 * sweep with common random numbers) join it and run as one kernel that computes each
 * activation's draws once for all of them (up to five points per lane at gamma = 0, two
 * otherwise, and adjacent lanes that run further points of the same episode and pass the
 * draws round: ten points in one launch at gamma = 0, eight otherwise); the summaries are the
 * same words as those of separate launches. The group is launched when it is full (one full
 * lane-group launch), before a call that does not join it is handled, and at the start of
 * every other entry point that takes the context or one of its batches; what is pending is
 * then cut into full lane-group launches first, the rest into groups of one lane's points,
 * a single call as its own launch. An error of a deferred launch is returned by the call
 * that triggers the launch. CPR_NAK_FUSE (read at every call) gives the most points per
 * lane; 0 or 1: every call launches at once. CPR_NAK_FUSE_LANES (read at every call) caps
 * the lanes per episode; 1: groups of one lane's points only, launched when those are
 * full. */
int cpr_run_episodes_async(cpr_batch* b, int64_t n_episodes, uint64_t first_episode,
                           cpr_summary* summary_dev, cpr_episode_record* records_dev);
int cpr_synchronize(cpr_ctx* ctx);
/* Replay trace episodes [0, trace->n_episodes) on the device with the batch's protocol,
 * mode and policy (fused episodes, like cpr_run_episodes, drawing from the trace instead
 * of the keyed stream); records[e] is trace episode e. summary (host) is accumulated (+=).
 * records: NULL or n_episodes records (device pointer if records_on_device != 0).
 * Replaces nothing in the reference directly: it is the cross-engine check the north star
 * asks for (same exported trace -> same per-episode outcomes). Synchronous. */
int cpr_replay(cpr_batch* b, const cpr_trace* trace, cpr_summary* summary,
               cpr_episode_record* records, int records_on_device);
/* Per-node outputs of episodes: activations per node and the head's reward array, one row
 * of n_nodes per episode (node 0 = the attacker on selfish-mining / two-agents networks;
 * n_nodes must be the network's node count: 2, defenders + 1, or defenders for cliques).
 * trace == NULL: keyed-stream episodes [first_episode, first_episode + n_episodes); else
 * trace episodes [0, trace->n_episodes) (n_episodes / first_episode ignored). The episodes
 * run on the exact event engine (Nakamoto configurations of the closed-form lane: the
 * Nakamoto-mode engine of its exact re-runs), so results equal cpr_run_episodes /
 * cpr_replay bit for bit. Host buffers: node_activations and node_rewards
 * [n_episodes][n_nodes]; records (optional) [n_episodes] as cpr_run_episodes, except that
 * head_miner is the head block's miner in LOOP mode too (nakamoto.ml:22-27 head info;
 * -1 genesis, Tailstorm summaries). Not for FC16. Synchronous. */
int cpr_node_outputs(cpr_batch* b, int64_t n_episodes, uint64_t first_episode,
                     const cpr_trace* trace, int32_t n_nodes, cpr_episode_record* records,
                     int64_t* node_activations, double* node_rewards);
/* device time (HIP events on the context's stream) of the last episode-kernel launch of
 * this batch, and the activations it simulated (valid after cpr_run_episodes returns;
 * after cpr_run_episodes_async the call launches a deferred launch, waits for the end of
 * the launch's kernel (also where the call was not deferred; the caller need not have
 * synchronized) and activations is -1; for a call that ran in a group of m the time is the
 * group's kernel time / m, so that the times of a sweep's points add up to the time of its
 * kernels on the context's stream. The eager second passes of a group with deferred races
 * run beside the next launch on the side stream and are not in that time) */
int cpr_last_launch(cpr_batch* b, double* kernel_ms, int64_t* activations);
/* shape of the last episode-kernel launch of this batch (fused episodes, replay, rollout):
 * lanes = device lanes launched; resident = lanes the device holds at once for that kernel
 * (occupancy API x CUs x 256, before the HBM budget and the episode count cap the launch).
 * Before any launch lanes = 0 and resident is the fused-episode kernel's figure.
 * Diagnostic for bench.py (lanes / resident), no reference counterpart. ABI v9. */
int cpr_launch_shape(cpr_batch* b, int64_t* lanes, int64_t* resident);
/* cumulative count of exact Nakamoto re-runs on this context whose episode outgrew the
 * LDS-resident event heap and ran again with the heap in HBM (k_nak_exact_rerun's second
 * attempt). Synchronizes the context's stream. Diagnostic, no reference counterpart. ABI v9. */
int cpr_rerun_hbm_retries(cpr_ctx* ctx, int64_t* retries);
/* cumulative exact re-runs on this context: episodes the fused kernels flagged (closed-form
 * Nakamoto overlaps, deep forks and unresolved ties; Ethereum window-lane hand-backs) and
 * re-ran on the exact event engine, the flushes that ran them and those flushes' kernel
 * milliseconds (HIP events on the context's stream). Synchronizes the stream if a flush is
 * pending. Diagnostic for bench.py, no reference counterpart. Since ABI v10. */
int cpr_rerun_stats(cpr_ctx* ctx, int64_t* episodes, int64_t* flushes, double* ms);
/* exact-replay coverage of this batch's lockstep lanes (Nakamoto closed-form lanes that
 * leave the closed form continue on the exact engine from an action log): log_steps = the
 * steps of each lane's action log, exact_slots = the engine slots shared by the lanes (both
 * 0 before the first cpr_reset, or where no lane can leave the closed form). A lane whose
 * episode is past log_steps, or that finds every slot taken, when it leaves the closed form
 * keeps the closed form's status flags (not exact); log_steps < max_steps happens only
 * beyond 4 GiB of logs (lanes x episode length). Diagnostic, no reference counterpart.
 * ABI v11. */
int cpr_lockstep_coverage(cpr_batch* b, int64_t* log_steps, int64_t* exact_slots);

/* Lockstep env API over cfg->n_lanes lanes (host pointers).
 * reset: lanes with mask[i] != 0 (mask NULL = all) start episode episode_ids[i]
 *        (episode_ids NULL = lane index); obs gets obs_len doubles per lane.
 * step:  actions[i] in [0, n_actions); writes obs, reward (engine.ml:223), done, info. */
int cpr_reset(cpr_batch* b, const uint8_t* mask, const uint64_t* episode_ids, double* obs);
int cpr_step(cpr_batch* b, const int32_t* actions, double* obs, double* reward,
             uint8_t* done, cpr_step_info* info);
/* integer observation fields of every lane: Nakamoto (public, private, diff, event);
 * B_k the 8 bk_ssz fields (bk_ssz.ml:22-34) */
int cpr_observe_fields(cpr_batch* b, int32_t* fields);

/* Lockstep rollout on the device (Nakamoto, Ethereum, B_k, Tailstorm; CPR_MODE_GYM batches
 * with n_lanes > 0): every one of cfg->n_lanes lanes takes n_steps
 * steps with the batch policy (cfg->policy, built-in or table) evaluated on the device;
 * a lane whose episode ends restarts at episode id (previous id + n_lanes), like a gym
 * VecEnv auto-reset (the observation written at a done step is the new episode's first).
 * Continues from the lanes' current state (a first call without cpr_reset starts lane i at
 * episode i). Outputs are optional, step-major:
 *   obs [n_steps][n_lanes][obs_len] f64, reward [n_steps][n_lanes] f64 (engine.ml:223),
 *   done [n_steps][n_lanes] u8; device pointers if outputs_on_device != 0, else host
 *   pointers (staged through library-owned device buffers).
 * summary (host, accumulated): steps / activations of the whole rollout, the other fields
 * over the episodes that finished in it. Synchronous; cpr_last_launch times the kernel.
 * Nakamoto: the closed-form lane on CPR_NET_SELFISH_MINING and CPR_NET_ABSTRACT_GAMMA with
 * the built-in policies and CPR_POLICY_TABLE (CPR_POLICY_RANDOM: CPR_E_UNSUPPORTED); a lane
 * whose step sets CPR_ST_LOCKSTEP_INEXACT bits continues on the exact engine as under
 * cpr_step (cpr_lockstep_coverage) until its episode ends, in further passes of the same
 * call: cpr_last_launch covers all of them, and more than n_steps + 1 rounds of passes is
 * CPR_E_STATE. cpr_step / cpr_reset may follow a rollout and the other way round.
 * Replaces SB3 SubprocVecEnv rollouts over cpr_gym envs (experiments/train/ppo.py:278-285). */
int cpr_rollout(cpr_batch* b, int64_t n_steps, double* obs, double* reward, uint8_t* done,
                int outputs_on_device, cpr_summary* summary);

/* Neural-network policies on the device (added within v11; nothing above changes).
 *
 * An actor-critic MLP as SB3's MlpPolicy builds it (experiments/train/ppo.py:400-416):
 * separate pi and vf trunks of `depth` hidden layers (1..CPR_POLICY_NET_MAX_DEPTH) with
 * ReLU after each, width_pi / width_vf units (multiples of 16 in [16, 512]), a linear
 * action head (n_actions of cpr_observation_spec) and a linear value head (1). The input
 * row is the lane's observation converted to f32 followed by the n_extra constants
 * extra[0..n_extra) (the alpha, gamma features of AssumptionScheduleWrapper, constant
 * within a batch unless cpr_lane_env_set names an alpha column). Weights are f32, row-major [out][in] like torch.nn.Linear: layer l of a
 * trunk is w[l] [width][l == 0 ? obs_len + n_extra : width], b[l] [width]; heads are
 * [n_actions][width_pi] and [1][width_vf]. All host pointers, copied by the call.
 * Arithmetic is f32 in, f32 accumulate on the matrix cores; argmax, sampling and the
 * log-probability are computed in f64 from the f32 logits l:
 *   deterministic: the lowest index of the maximum logit
 *   sampled: m = max l, e_i = exp(l_i - m), S = sum e_i in index order, action = the
 *     smallest a with u S < sum_{i <= a} e_i (the last action if rounding leaves none),
 *     u = u53(w0, w1) of the keyed block ctr = (episode, i, 0x60000000), key = seed, i = the
 *     episode step index before the step: a draw depends on (seed, episode, step) only
 *   logp = l_a - m - log S */
#define CPR_POLICY_NET_MAX_DEPTH 4
#define CPR_POLICY_NET_MAX_EXTRA 8
typedef struct cpr_policy_net {
  int32_t n_extra;
  float extra[CPR_POLICY_NET_MAX_EXTRA];
  int32_t depth;
  int32_t width_pi;
  int32_t width_vf;
  const float* pi_w[CPR_POLICY_NET_MAX_DEPTH];
  const float* pi_b[CPR_POLICY_NET_MAX_DEPTH];
  const float* pi_head_w;
  const float* pi_head_b;
  const float* vf_w[CPR_POLICY_NET_MAX_DEPTH];
  const float* vf_b[CPR_POLICY_NET_MAX_DEPTH];
  const float* vf_head_w;
  const float* vf_head_b;
} cpr_policy_net;

/* Set (or replace) the batch's network: shapes are checked against the batch, weights must
 * be finite. CPR_E_UNSUPPORTED: FC16, a batch without lanes (n_lanes = 0), or a
 * configuration whose workgroup tile needs more LDS than the device has (the widest trunk
 * decides; two hidden tiles from depth 2 on) -- refused here, never
 * launched. */
int cpr_policy_net_set(cpr_batch* b, const cpr_policy_net* net);
/* The network on n >= 1 observation rows (host buffers, obs [n][obs_len]); every output is
 * optional: actions [n], logp [n], value [n], logits [n][n_actions]. Sampled mode
 * (deterministic == 0) draws row r at (episode episode0 + r, step 0). CPR_E_STATE without a
 * network. Synchronous. */
int cpr_policy_net_forward(cpr_batch* b, const double* obs, int64_t n, int deterministic,
                           uint64_t episode0, int32_t* actions, double* logp, double* value,
                           float* logits);

/* outputs of a network rollout; every pointer optional, step-major */
typedef struct cpr_rollout_net_out {
  double* obs0;    /* [n_lanes][obs_len] the observation before the first step */
  double* obs;     /* [n_steps][n_lanes][obs_len] after step t (after a done: the new
                      episode's first); the policy input of step t is obs0 / obs[t-1] */
  int32_t* action; /* [n_steps][n_lanes] */
  double* reward;  /* [n_steps][n_lanes] engine.ml:223 */
  uint8_t* done;   /* [n_steps][n_lanes] */
  double* logp;    /* [n_steps][n_lanes] log-probability of the action taken */
  double* value;   /* [n_steps + 1][n_lanes] value of the policy input of step t; row n_steps
                      is the value of the final observation (PPO's bootstrap) */
} cpr_rollout_net_out;

/* Lockstep rollout driven by the batch's network: per step, on the context's stream, the
 * network forward on the lanes' observations, the protocol's lockstep step kernels (for
 * Nakamoto the exact pass too: lanes that leave the closed form continue on the exact
 * engine as under the host-driven step), the bookkeeping kernel and the protocol's reset
 * kernel with a device mask; no host synchronisation until the end. Semantics as the
 * built-in rollout above: continues from the lanes' state (a first call without a reset
 * starts lane i at episode i), auto-reset at episode id + n_lanes, summary accumulated the
 * same way; out may be NULL; device pointers if outputs_on_device != 0. The host-driven
 * step, reset and the built-in rollout may follow and precede it. Sampled draws of a lane
 * depend on (seed, episode, step) only, so chunking a rollout into calls changes nothing.
 * CPR_E_STATE without a network. Synchronous; the launch timer covers the whole call. */
int cpr_rollout_net(cpr_batch* b, int64_t n_steps, int deterministic,
                    const cpr_rollout_net_out* out, int outputs_on_device,
                    cpr_summary* summary);

/* The gym layers of cpr-v0 over the lockstep lanes (added within v11; a batch on which
 * cpr_lane_env_set was never called behaves exactly as before). gym/ocaml/cpr_gym/envs.py:99-191
 * wraps core-v0 in an assumption schedule (an alpha per episode, appended to the observation),
 * a reward wrapper and a normalisation; experiments/train/ppo.py:105-141,200-270 schedules
 * alpha per episode and shapes the reward. Here:
 *
 * Assumption schedule. The batch holds a table of n_alpha alphas. Episode e runs at entry
 *   min(n_alpha - 1, (int)(u n_alpha)), u = u53(w0, w1) of the keyed block
 *   ctr = (e, 0, 0x70000000), key = seed
 * (random.choice over a list, ppo.py:117-118; a range is served by a table of grid points
 * or of pre-drawn values): an episode's alpha depends on (seed, episode) only, not on the
 * lane count or on how a rollout is cut into calls. The table is converted to miner-draw
 * thresholds like cfg.alpha, so a one-entry table equal to cfg.alpha changes nothing.
 * Gamma, defenders and delays stay the batch's. The per-lane alpha holds in cpr_reset,
 * cpr_step, cpr_observe_fields and cpr_rollout_net (the exact-engine continuation of
 * Nakamoto lanes included). Fused episodes (cpr_run_episodes), cpr_replay and
 * cpr_node_outputs of the same batch keep cfg.alpha.
 *
 * Network input. In a network rollout, extra column alpha_column of the network's input is
 * the row's lane alpha rounded to f32 instead of the constant extra[alpha_column]; the other
 * extras stay constants. extra = (alpha, gamma) with alpha_column = 0 is
 * AssumptionScheduleWrapper's layout (wrappers.py:172-242); alpha_column = -1 leaves every
 * extra constant (its pretend_alpha). cpr_policy_net_forward works on host rows that belong
 * to no lane and keeps using the constants.
 *
 * Rewards of a network rollout (f64, one rounding per operation, from the step infos):
 *   CPR_GYM_REWARD_ENGINE              engine.ml:223, unchanged
 *   CPR_GYM_REWARD_SPARSE_RELATIVE     0 until done, then ra / (ra + rd), 0 if the sum is 0
 *                                      (wrappers.py:8-26)
 *   CPR_GYM_REWARD_SPARSE_PER_PROGRESS 0 until done, then ra / progress, 0 if progress is 0
 *                                      (wrappers.py:29-51)
 *   CPR_GYM_REWARD_DENSE_PER_PROGRESS  r * (1 / dense_target) per step, summed per lane since
 *                                      its reset (acc); at a done with progress != dense_target
 *                                      the reward gains (dense_target - progress) * acc /
 *                                      progress (wrappers.py:54-113; nothing where progress
 *                                      is 0: the reference raises there). The accumulator
 *                                      follows network rollouts and resets only: steps taken
 *                                      through cpr_step or cpr_rollout are not added
 * then the shape:
 *   CPR_SHAPE_NONE       r
 *   CPR_SHAPE_PER_ALPHA  r / alpha of the lane (envs.py:149-150, ppo.py `raw`)
 *   CPR_SHAPE_CUT        0 if r <= 0 or progress <= 0; (r * 0.9) / alpha if n_activations /
 *                        progress <= 1.05; else r / alpha (ppo.py:221-232)
 * ppo.py's `exp` shape is left to the caller (numpy.exp is not pinned bit for bit): the
 * unshaped reward and the alpha are among the outputs. cpr_step's reward stays the engine's. */
enum cpr_gym_reward {
  CPR_GYM_REWARD_ENGINE = 0,
  CPR_GYM_REWARD_SPARSE_RELATIVE = 1,
  CPR_GYM_REWARD_SPARSE_PER_PROGRESS = 2,
  CPR_GYM_REWARD_DENSE_PER_PROGRESS = 3
};
enum cpr_reward_shape { CPR_SHAPE_NONE = 0, CPR_SHAPE_PER_ALPHA = 1, CPR_SHAPE_CUT = 2 };
#define CPR_LANE_ENV_MAX_ALPHA 4096
typedef struct cpr_lane_env {
  int32_t n_alpha;       /* 1..CPR_LANE_ENV_MAX_ALPHA table entries; 0 with alpha = NULL: */
  const double* alpha;   /* cfg.alpha for every lane. Host pointer, copied by the call */
  int32_t alpha_column;  /* extras column fed with the lane's alpha; -1 none */
  int32_t gym_reward;    /* enum cpr_gym_reward */
  int32_t reward_shape;  /* enum cpr_reward_shape */
  double dense_target;   /* CPR_GYM_REWARD_DENSE_PER_PROGRESS: episode_len (> 0) */
} cpr_lane_env;
/* Set the batch's lane env, before its first reset or rollout (CPR_E_STATE afterwards).
 * CPR_E_INVALID_ARG: n_alpha out of range; an alpha that is NaN or outside [0, 1], or outside
 * (0, 1] with a shape that divides by it; dense_target <= 0 with the dense reward;
 * alpha_column < -1, or >= n_extra of the batch's network (checked by whichever of this call
 * and cpr_policy_net_set comes second). CPR_E_UNSUPPORTED: FC16, a batch without lockstep
 * lanes. While a table is set (n_alpha > 0), cpr_rollout (built-in policies) is
 * CPR_E_UNSUPPORTED. */
int cpr_lane_env_set(cpr_batch* b, const cpr_lane_env* env);
/* alpha of every lane's current episode ([n_lanes], host): cfg.alpha without a lane env or
 * before the first reset; the Python wrappers' info["alpha"] */
int cpr_lane_alpha(cpr_batch* b, double* alpha);
/* further outputs of a network rollout; every pointer optional */
typedef struct cpr_rollout_env_out {
  double* alpha0;        /* [n_lanes] alpha of the episode obs0 belongs to */
  double* alpha;         /* [n_steps][n_lanes] alpha of the episode obs[t] belongs to */
  double* engine_reward; /* [n_steps][n_lanes] the unwrapped engine.ml:223 reward */
} cpr_rollout_env_out;
/* cpr_rollout_net with those outputs (env_out may be NULL: the same call). Once a lane env
 * is set, out->reward of either call is the wrapped and shaped reward. cpr_summary is
 * computed as before. */
int cpr_rollout_net_env(cpr_batch* b, int64_t n_steps, int deterministic,
                        const cpr_rollout_net_out* out, const cpr_rollout_env_out* env_out,
                        int outputs_on_device, cpr_summary* summary);
/* Whether the batch's last cpr_rollout_net / _env (cpr_ppo_iterate's included) ran its steps in
 * one kernel (added within v11). CPR_PROTO_FC16_ENV batches do when the environment variable
 * CPR_FC16_ROLLOUT_FUSED=1 is set (read at every call) and the kernel's LDS fits the device,
 * with the same outputs bit for bit as the launch sequence that every protocol runs by default
 * (CPR_FC16_ROLLOUT_FUSED=0 or unset): forward, step, collect and reset kernels per step. The
 * one-kernel path is faster at a few thousand lanes and slower at 65,536 lanes with a 3 x 64
 * network, hence off by default. */
int cpr_rollout_net_fused(cpr_batch* b, int32_t* fused);

/* A cyclic assumption schedule (added within v11; a batch that never calls this launches what
 * it did before). CPR_SCHEDULE_CHOICE is the keyed random.choice above. Under
 * CPR_SCHEDULE_CYCLE episode e runs at table entry e mod n_alpha: itertools.cycle over the
 * table (AssumptionScheduleWrapper, wrappers.py:186-193) as a function of the episode id
 * alone, so it depends neither on the lane count nor on how a run is cut into calls.
 * Everything that follows the lane alpha follows it under either schedule. Callable when
 * cpr_lane_env_set is: before the batch's first reset or rollout (CPR_E_STATE afterwards);
 * cpr_lane_env_set keeps the schedule. CPR_E_INVALID_ARG: an unknown schedule. */
enum cpr_alpha_schedule { CPR_SCHEDULE_CHOICE = 0, CPR_SCHEDULE_CYCLE = 1 };
int cpr_lane_env_schedule(cpr_batch* b, int schedule);

/* Evaluation of the batch's network (added within v11): EvalCallback + evaluate_policy of
 * experiments/train/ppo.py:296-374,421-450 and experiments/rl-eval. A fixed set of whole
 * episodes, one result per alpha.
 *
 * Episode set. A = the lane env's n_alpha (1 without a lane env: cfg.alpha). The set is
 * [first_episode, first_episode + A episodes_per_alpha); under CPR_SCHEDULE_CYCLE every
 * alpha gets exactly episodes_per_alpha of them. The call resets every lane (lane i to
 * episode first_episode + i), then steps all lanes with the network; a lane whose episode ends
 * restarts at its id + n_lanes, as in the rollout, also beyond the set (whatever episodes
 * outside the set produce is discarded). The call ends when every episode of the set has
 * finished: the host reads a device counter every check_every steps (0: every max_steps
 * steps). ceil(set / n_lanes) max_steps steps always suffice; a counter that disagrees after
 * that many is CPR_E_INTERNAL. The results depend on the seed, the set and the network only,
 * not on n_lanes or check_every.
 *
 * One record per episode of the set, at slot episode - first_episode: the reward is the wrapped
 * and shaped reward of the lane env (the engine's without one) summed in step order from 0
 * (EpisodeRecorderWrapper's erw_episode_reward, wrappers.py:245-266); the other fields are
 * the step infos of the episode's last step. height is the head height the summary's orphans
 * are counted against (B_k, Tailstorm: (int64)progress).
 *
 * Per alpha (entry j of the table; slots s with (first_episode + s) mod A = j, in slot order
 * r_0, r_1, ...): a cpr_summary of those records by the rule of every other summary (an
 * episode with CPR_ST_INVALID bits: steps, activations and `invalid` only), and the mean and
 * unbiased standard deviation of the five columns EvalCallback logs, over the n valid records,
 * in f64 with this order (one rounding per operation, no fused multiply-add):
 *   p_t = 0 + sum of x(r_k) over valid r_k, k = t, t + 256, t + 512, ... in that order, t < 256
 *   for off = 128, 64, ..., 1: p_t = p_t + p_{t + off} for every t < off
 *   mean = p_0 / n
 *   the same with (x(r_k) - mean) (x(r_k) - mean) in place of x(r_k): std = sqrt(p_0 / (n - 1))
 * mean is NaN for n = 0 and std for n < 2 (pandas). x of column CPR_EVAL_N_ACTIVATIONS is
 * (double)episode_n_activations.
 *
 * CPR_E_STATE without a network; CPR_E_INVALID_ARG: episodes_per_alpha < 1, check_every < 0;
 * CPR_E_UNSUPPORTED: FC16, cfg.max_steps <= 0 (no bound on an episode), a table of more than
 * one alpha under CPR_SCHEDULE_CHOICE (its alphas do not get equal shares of a set). After
 * the call the lanes stand in arbitrary later episodes: cpr_step, cpr_rollout and
 * cpr_rollout_net are CPR_E_STATE until a cpr_reset of every lane or the next cpr_eval_net.
 * Weights, Adam state and the update count are untouched. Synchronous; the launch timer
 * covers the whole call. */
typedef struct cpr_eval_opts {
  int64_t episodes_per_alpha; /* >= 1 */
  uint64_t first_episode;
  int32_t deterministic;      /* EvalCallback: 1 */
  int64_t check_every;        /* steps between looks at the finished-episode counter; 0: max_steps */
} cpr_eval_opts;
typedef struct cpr_eval_record {
  uint64_t episode;
  double alpha;
  double episode_reward;
  double episode_sim_time;
  double episode_chain_time;
  double episode_progress;
  double reward_attacker;
  double reward_defender;
  int64_t episode_n_activations;
  int64_t episode_n_steps;
  int64_t height;
  int32_t alpha_index;
  uint32_t status;            /* enum cpr_episode_status bits */
} cpr_eval_record;
enum cpr_eval_column {
  CPR_EVAL_REWARD = 0, CPR_EVAL_SIM_TIME = 1, CPR_EVAL_CHAIN_TIME = 2, CPR_EVAL_PROGRESS = 3,
  CPR_EVAL_N_ACTIVATIONS = 4
};
#define CPR_EVAL_COLUMNS 5
typedef struct cpr_eval_alpha {
  double alpha;
  int64_t n;                  /* valid episodes */
  double mean[CPR_EVAL_COLUMNS];
  double std[CPR_EVAL_COLUMNS];
} cpr_eval_alpha;
/* Host pointers: records NULL or [A episodes_per_alpha]; per_alpha [A]; per_alpha_summary
 * NULL or [A] (overwritten); total NULL or one summary (overwritten): the field-wise sum of
 * the per-alpha summaries. */
int cpr_eval_net(cpr_batch* b, const cpr_eval_opts* opts, cpr_eval_record* records,
                 cpr_eval_alpha* per_alpha, cpr_summary* per_alpha_summary, cpr_summary* total);

/* The weights of src into dst, device to device on the context's stream, no host round trip:
 * the reference's separate eval_env (ppo.py:421-450) takes the training batch's weights this
 * way. Both batches belong to one context. A dst without a network acquires src's shapes
 * (checked like cpr_policy_net_set, the LDS check included); otherwise depth, widths, n_extra
 * and the extras must be equal (CPR_E_INVALID_ARG; so are different observation or action
 * widths and different contexts). dst's Adam state and update count are zeroed as after
 * cpr_policy_net_set; src is unchanged. CPR_E_STATE: src has no network. */
int cpr_policy_net_copy(cpr_batch* dst, cpr_batch* src);

/* The learner (added within v11; a batch that never calls these launches what it did before):
 * SB3's PPO.train (experiments/train/ppo.py:399-451) on the batch's device weights.
 * DESIGN.md §4.14 "Learner" has the loss, its derivative and every reduction order.
 *
 * cpr_gae: RolloutBuffer.compute_returns_and_advantage over step-major f64 buffers of the
 * batch's n_lanes: reward, done [n_steps][n_lanes], value [n_steps + 1][n_lanes] (row n_steps
 * the bootstrap) -> adv_out, ret_out [n_steps][n_lanes]. Per lane, t = n_steps - 1 .. 0, one
 * rounding per operation:
 *   nnt = 1 - done[t];  delta = (reward[t] + (gamma value[t + 1]) nnt) - value[t]
 *   last = delta + ((gamma lam) nnt) last;  adv[t] = last;  ret[t] = last + value[t]
 * (value[t + 1] at a done step is the reset observation's value, masked by nnt; no
 * time-limit bootstrap). Host pointers, or device pointers if on_device != 0. */
int cpr_gae(cpr_batch* b, int64_t n_steps, const double* reward, const uint8_t* done,
            const double* value, double gamma, double lam, double* adv_out, double* ret_out,
            int on_device);

typedef struct cpr_ppo_opts {
  int32_t n_epochs;            /* >= 1 */
  int64_t minibatch;           /* >= 1 rows; an epoch's last minibatch may be shorter */
  double clip_range;
  double ent_coef;
  double vf_coef;
  double max_grad_norm;
  double lr;                   /* per call: the caller applies its schedule */
  double beta1, beta2, adam_eps;
  int32_t normalize_advantage; /* per minibatch, (A - mean) / (std + 1e-8), unbiased std */
  double gae_gamma, gae_lambda; /* cpr_ppo_iterate */
  uint64_t perm_seed;
} cpr_ppo_opts;
/* the reference's values (ppo.py:399-417 over SB3's defaults): 10 epochs, minibatch 64,
 * clip 0.1, ent 0, vf 0.5, max-norm 0.5, lr 3e-4, betas (0.9, 0.999), eps 1e-5, normalised
 * advantages, gamma 0.99, lambda 0.95, perm_seed 0 */
int cpr_ppo_opts_default(cpr_ppo_opts* opts);

/* n rows of training data (the flat [n_steps * n_lanes] rollout buffers): the policy input of
 * every row, its lane alpha (read only when the batch's lane env names an alpha column), the
 * action taken, its log-probability then, the advantage and the return. Host pointers, or
 * device pointers if on_device != 0; rows_idx / perm of the calls below follow the same flag. */
typedef struct cpr_ppo_data {
  int64_t n;
  const double* obs;       /* [n][obs_len] */
  const double* alpha;     /* [n] or NULL */
  const int32_t* action;   /* [n] */
  const double* old_logp;  /* [n] */
  const double* advantage; /* [n] */
  const double* ret;       /* [n] */
  int32_t on_device;
} cpr_ppo_data;

/* SB3's logged statistics: row means of a minibatch, or their mean over an update's minibatches */
typedef struct cpr_ppo_stats {
  double policy_loss;   /* mean(-min(A rho, A clamp(rho, 1 - c, 1 + c))) */
  double value_loss;    /* mean((R - v)^2) */
  double entropy_loss;  /* mean(-H) */
  double approx_kl;     /* mean((rho - 1) - log rho) */
  double clip_fraction; /* mean(|rho - 1| > c) */
  double loss;          /* policy_loss + ent_coef entropy_loss + vf_coef value_loss */
  double grad_norm;     /* global L2 norm before the clip */
  int64_t n_minibatches;
} cpr_ppo_stats;

/* The gradient of one minibatch (rows rows_idx[0 .. n_rows) of data, int32) and its statistics;
 * the weights stay. grad_out (host): a flat f32 vector, for the pi trunk then the vf trunk:
 * each hidden layer's W [out][in] then b, then the head's W and b -- cpr_ppo_param_count
 * floats. stats_out may be NULL. Synchronous. CPR_E_STATE without a network;
 * CPR_E_UNSUPPORTED if the training kernels' tile exceeds the device's LDS (refused before
 * any launch); CPR_E_INVALID_ARG names the offending field. */
int cpr_ppo_gradients(cpr_batch* b, const cpr_ppo_data* data, const int32_t* rows_idx,
                      int64_t n_rows, const cpr_ppo_opts* opts, float* grad_out,
                      cpr_ppo_stats* stats_out);
int cpr_ppo_param_count(cpr_batch* b, int64_t* count);

/* n_epochs x ceil(n / minibatch) steps of gradient, global-norm clip and Adam on the batch's
 * device weights, no host synchronisation between them. perm: int32 [n_epochs][n], each row a
 * permutation of 0 .. n - 1 (minibatch k of epoch e is perm[e][k minibatch ..]). perm == NULL:
 * the library draws epoch e's permutation by Fisher-Yates from the keyed stream,
 *   for i = n - 1 .. 1: swap(p[i], p[min(i, (int)(u (i + 1)))]), u = u53 of words 2 (i & 1), + 1
 *   of block ctr = (update count, e, i >> 1, 0x80000000), key = seed ^ perm_seed * 0x9E3779B97F4A7C15
 * where the update count is the number of cpr_ppo_update calls on this batch since
 * cpr_policy_net_set. Adam's m, v and step count belong to the batch and are zeroed by
 * cpr_policy_net_set. stats_out (optional): means over the minibatches. Synchronous. */
int cpr_ppo_update(cpr_batch* b, const cpr_ppo_data* data, const cpr_ppo_opts* opts,
                   const int32_t* perm, cpr_ppo_stats* stats_out);

/* One PPO iteration: cpr_rollout_net_env (sampled) of n_steps into rollout buffers the batch
 * owns on the device, cpr_gae (opts->gae_gamma, gae_lambda), cpr_ppo_update (perm NULL) on the
 * n_steps * n_lanes rows. Bit for bit what the three calls give when composed by hand. */
int cpr_ppo_iterate(cpr_batch* b, int64_t n_steps, const cpr_ppo_opts* opts,
                    cpr_summary* summary, cpr_ppo_stats* stats_out);

/* Q-learning (added within v11; a batch that never calls these launches what it did before):
 * SB3's DQN as gym/rust/hyperparams/dqn.yml configures it, on the batch's device weights.
 * DESIGN.md §4.14 "Q-learning" has the loss, every order and the deviations from SB3.
 *
 * The Q-network is the batch's policy network: Q(s, a) = logit a of the pi trunk and its head.
 * The vf trunk takes no part: the DQN kernels skip it, its gradient is exactly zero and its
 * weights keep their bytes. The greedy policy is deterministic = 1 of the existing forward.
 * Adam's moments and step count are the learner's (shared with cpr_ppo_update). */
typedef struct cpr_dqn_opts {
  int64_t batch;                  /* >= 1 rows per gradient step */
  int32_t gradient_steps;         /* >= 0 per cpr_dqn_iterate */
  double gamma;
  double lr;
  double beta1, beta2, adam_eps;
  double max_grad_norm;
  double tau;                     /* cpr_dqn_iterate's Polyak weight, in [0, 1] */
  int64_t target_update_interval; /* in transitions; / n_lanes in vector steps */
  int64_t learning_starts;        /* in transitions */
  uint64_t sample_seed;
} cpr_dqn_opts;
/* dqn.yml's default block over SB3's: batch 32, 1 gradient step, gamma 0.99, lr 1e-4, betas
 * (0.9, 0.999), eps 1e-8, max-norm 10, tau 1, interval 10,000, learning_starts 50,000, seed 0 */
int cpr_dqn_opts_default(cpr_dqn_opts* opts);

/* n transitions: the policy input, the lane alpha of the row (read only when the batch's lane
 * env names an alpha column; it is next_obs' alpha too), the action, the reward, done and the
 * next policy input. Host pointers, or device pointers if on_device != 0. */
typedef struct cpr_dqn_data {
  int64_t n;
  const double* obs;      /* [n][obs_len] */
  const double* alpha;    /* [n] or NULL */
  const int32_t* action;  /* [n] */
  const double* reward;   /* [n] */
  const uint8_t* done;    /* [n] */
  const double* next_obs; /* [n][obs_len] */
  int32_t on_device;
} cpr_dqn_data;

/* row means of a gradient step, or their mean over an update's steps (stream order) */
typedef struct cpr_dqn_stats {
  double loss;      /* mean smooth_l1(q_a - y), beta = 1 */
  double abs_td;    /* mean |q_a - y| */
  double q;         /* mean q_a */
  double target;    /* mean y */
  double grad_norm; /* global L2 norm before the clip */
  int64_t n_steps;  /* gradient steps behind the means; 0: no update ran */
} cpr_dqn_stats;

/* The replay ring: capacity_steps slots of n_lanes transitions (SB3's buffer_size // n_envs),
 * the inputs stored in f32 (the forward rounds to f32 first, so a stored row gives the Q-values
 * of the original f64 row bit for bit). The target network becomes a copy of the weights; the
 * slot cursor, the size, the counts of collected steps and of updates, and Adam's state are
 * zeroed. CPR_E_STATE without a network; CPR_E_UNSUPPORTED where cpr_policy_net_set is;
 * capacity_steps < 1 is CPR_E_INVALID_ARG. A later cpr_policy_net_set / _copy keeps the ring and
 * makes the target a copy of the new weights. */
int cpr_dqn_init(cpr_batch* b, int64_t capacity_steps);

/* cpr_rollout_net_env's per-step launch sequence (forward, step kernels, collect, masked reset;
 * never the one-kernel FC16 rollout) with an epsilon-greedy action: of the keyed block
 * ctr = (episode, episode step index before the step, 0x90000000), key = seed,
 * u1 = u53(w0, w1), u2 = u53(w2, w3); u1 < epsilon: min(n_actions - 1, (int)(u2 n_actions)),
 * else the lowest index of the maximum. Step t of the call goes to slot (cursor + t) mod
 * capacity; size = min(capacity, size + n_steps). The reward is the lane env's if one is set;
 * next_obs is the observation after the step's auto-reset. epsilon = 0 is
 * cpr_rollout_net_env(deterministic = 1) bit for bit. One synchronisation, at the end. */
int cpr_dqn_collect(cpr_batch* b, int64_t n_steps, double epsilon, cpr_summary* summary);

/* The gradient of one minibatch (rows rows_idx[0 .. n_rows) of data, int64; a device pointer if
 * data->on_device) and its statistics; the weights stay. Needs cpr_dqn_init (the target). grad_out: cpr_ppo_gradients' flat order, cpr_ppo_param_count floats (the vf
 * trunk's are zero). Only opts->gamma is read. Per row, f64, one rounding per operation:
 *   q' = max_i target(next_obs)_i;  y = reward + (gamma q') (1 - done);  d = q_a - y
 *   l = 0.5 d^2 if |d| < 1 else |d| - 0.5;  dL/dq_a = clamp(d, -1, 1) / n_rows */
int cpr_dqn_gradients(cpr_batch* b, const cpr_dqn_data* data, const int64_t* rows_idx,
                      int64_t n_rows, const cpr_dqn_opts* opts, float* grad_out,
                      cpr_dqn_stats* stats_out);

/* gradient_steps steps of gradient (opts->batch rows of the ring), global-norm clip and Adam, no
 * host synchronisation between them. idx: int64 [gradient_steps][batch] flat transition
 * indices slot * n_lanes + lane (host), each < size * n_lanes. idx == NULL: row i of step g of
 * update U (the count of cpr_dqn_update calls since cpr_dqn_init / cpr_policy_net_set) is
 *   min(n - 1, (int64)(u n)), n = size * n_lanes, u = u53 of words 2 (i & 1), + 1 of block
 *   ctr = (U, g, i >> 1, 0xA0000000), key = seed ^ sample_seed * 0x9E3779B97F4A7C15
 * CPR_E_STATE: no cpr_dqn_init, or an empty ring. gradient_steps = 0 does nothing. */
int cpr_dqn_update(cpr_batch* b, int32_t gradient_steps, const cpr_dqn_opts* opts,
                   const int64_t* idx, cpr_dqn_stats* stats_out);
/* the indices the last cpr_dqn_update read, copied back from the device: the first n of
 * [gradient_steps][batch] */
int cpr_dqn_last_indices(cpr_batch* b, int64_t* out, int64_t n);

/* SB3's polyak_update, elementwise in f32: t = (t omt) + (p tf), omt = (float)(1 - tau),
 * tf = (float)tau, one rounding per product and one for the sum; tau = 1 copies the bytes. */
int cpr_dqn_target_sync(cpr_batch* b, double tau);

/* cpr_dqn_collect; then cpr_dqn_target_sync(opts->tau) once if the batch's collected vector
 * steps crossed a multiple of max(target_update_interval / n_lanes, 1) during it; then
 * cpr_dqn_update(opts->gradient_steps, idx NULL) if the collected transitions have reached
 * learning_starts (else stats_out->n_steps = 0). Bit for bit the three calls by hand. */
int cpr_dqn_iterate(cpr_batch* b, int64_t n_steps, double epsilon, const cpr_dqn_opts* opts,
                    cpr_summary* summary, cpr_dqn_stats* stats_out);

/* Slots [first_slot, first_slot + n_slots) of the ring into out's arrays (host, writable
 * despite the const; alpha may be NULL), n_slots * n_lanes rows. Slot `capacity_steps` is a
 * guard slot behind the ring that no collect writes (cpr_dqn_init fills it with 0xA5 bytes).
 * size / cursor / capacity (optional): the ring's state in slots. */
int cpr_dqn_replay_get(cpr_batch* b, int64_t first_slot, int64_t n_slots, cpr_dqn_data* out);
int cpr_dqn_replay_state(cpr_batch* b, int64_t* size, int64_t* cursor, int64_t* capacity);
/* the target network, as cpr_policy_net_get */
int cpr_dqn_target_get(cpr_batch* b, cpr_policy_net* net);

/* The batch's current weights into the caller's arrays, laid out as for cpr_policy_net_set
 * (every array pointer of `net` must be writable despite the const; n_extra, extra, depth
 * and the widths are filled in). */
int cpr_policy_net_get(cpr_batch* b, cpr_policy_net* net);

/* policy evaluated on encoded observations (host): obs n x obs_len -> actions n */
int cpr_policy_actions(cpr_batch* b, int32_t policy, const double* obs, int64_t n,
                       int32_t* actions);

int cpr_observation_spec(cpr_batch* b, int32_t* obs_len, int32_t* n_actions, double* low,
                         double* high);
/* policy names in the reference's registry order (Collection prepends): index -> name */
int cpr_policy_count(int32_t protocol);
const char* cpr_policy_name(int32_t protocol, int32_t index, int32_t* policy_id);

/* Keyed stream: out[4*i..4*i+3] = Philox4x32-10 block of
 * ctr = (episode_lo, episode_hi, idx0 + i, tag), key = (seed_lo, seed_hi), computed on
 * the device; exp_out (optional) = -log(u53(w2,w3)) of each block via cpr_log. */
int cpr_stream_fill(cpr_ctx* ctx, uint64_t seed, uint64_t episode, uint32_t idx0,
                    uint32_t tag, int64_t n, uint32_t* out, double* exp_out);

/* Value iteration over explicit MDPs (additive within ABI v11; mdp/lib/explicit_mdp.py:97-177
 * on the device). P points share one topology in the dense padded form: S states,
 * A action slots per state, T transition slots per action; a point is one probability array.
 * Host pointers. */
typedef struct cpr_mdp {
  int32_t S, A, T, P;
  const int32_t* dst;   /* [S][A][T] destination state of a used slot */
  const uint8_t* used;  /* [S][A][T] 0: a padding slot, whatever else it holds is ignored */
  const uint8_t* valid; /* [S][A]    0: the state does not offer that action */
  const double* rew;    /* [S][A][T] */
  const double* prg;    /* [S][A][T] */
  const double* prb;    /* [P][S][A][T] */
} cpr_mdp;

enum cpr_mdp_vi_path { CPR_MDP_VI_AUTO = 0, CPR_MDP_VI_RESIDENT = 1, CPR_MDP_VI_GLOBAL = 2 };
enum cpr_mdp_vi_status {
  CPR_MDP_VI_CONVERGED = 0,    /* the last sweep's delta <= stop_delta */
  CPR_MDP_VI_MAX_ITER = 1,     /* stopped after sweep max_iter */
  CPR_MDP_VI_NOT_CONVERGED = 2 /* max_iter == 0 and the library's sweep cap was reached: 2^20,
                                  or the lower value of the environment variable
                                  CPR_MDP_VI_SWEEP_CAP (a test hook) */
};

typedef struct cpr_mdp_vi_opts {
  double stop_delta; /* >= 0 */
  double discount;   /* in (0, 1] */
  int64_t max_iter;  /* >= 0; 0: until delta <= stop_delta (then stop_delta must be > 0) */
  int32_t path;      /* enum cpr_mdp_vi_path; AUTO: resident if the states fit one workgroup
                        and its estimated sweep time is the lower one */
} cpr_mdp_vi_opts;
/* stop_delta 1e-6, discount 1, max_iter 0, path AUTO */
int cpr_mdp_vi_opts_default(cpr_mdp_vi_opts* opts);

typedef struct cpr_mdp_vi_result {
  double* value;    /* [P][S] */
  double* progress; /* [P][S] */
  int32_t* policy;  /* [P][S] the action slot taken, -1 for a state without valid action */
  int64_t* iter;    /* [P] sweeps done */
  double* delta;    /* [P] max |value - previous value| of the last sweep */
  int32_t* status;  /* [P] enum cpr_mdp_vi_status */
  int32_t path_used; /* CPR_MDP_VI_RESIDENT or CPR_MDP_VI_GLOBAL */
  double kernel_ms;  /* HIP events around the launches, the status reads between them included */
} cpr_mdp_vi_result;

/* Per point: value = progress = 0; sweep i computes, per state and valid action in slot order,
 * this_v += prb (rew + discount value[dst]) and this_p likewise over the used slots in slot
 * order (f64, one rounding per operation), takes an action when this_v > best_v or none is
 * taken yet, and gives a state without valid action value 0, progress 0, policy -1. The point
 * stops after sweep i if max_iter > 0 and i >= max_iter, else if delta <= stop_delta; points
 * stop independently. Every array of `result` is filled. Checked before anything is launched
 * (CPR_E_INVALID_ARG): sizes < 1, NULL arrays, a used dst outside [0, S), a non-finite prb, rew
 * or prg in a used slot, discount outside (0, 1], stop_delta < 0, max_iter < 0, stop_delta == 0
 * with max_iter == 0, an unknown path. A used slot is checked even under an action with
 * valid == 0, although no solver takes that action. CPR_E_CAPACITY: no host memory for the
 * upload copies; path RESIDENT with more states than one
 * workgroup holds (about 10,000). */
int cpr_mdp_value_iteration(cpr_ctx* ctx, const cpr_mdp* mdp, const cpr_mdp_vi_opts* opts,
                            cpr_mdp_vi_result* result);

/* Policy evaluation over explicit MDPs (additive within ABI v11; mdp/lib/explicit_mdp.py:328-378
 * and :179-208 on the device). A job holds E evaluations over one cpr_mdp: each
 * plays its own policy at one of the P points. A cross product, a diagonal or a ragged selection
 * of (policy, point) pairs are all this one form. Host pointers. */
enum cpr_mdp_pe_states {
  CPR_MDP_PE_REACHABLE = 0, /* the states the policy reaches from the start states (the
                               reference's around_state = None) */
  CPR_MDP_PE_ALL = 1        /* every state (the reference's around_state given) */
};
enum cpr_mdp_pe_status {
  CPR_MDP_PE_CONVERGED = 0,    /* the last sweep's delta < theta */
  CPR_MDP_PE_MAX_ITER = 1,     /* stopped after sweep max_iter */
  CPR_MDP_PE_NOT_CONVERGED = 2 /* max_iter == 0 and the library's sweep cap was reached: 2^20,
                                  or the lower value of the environment variable
                                  CPR_MDP_PE_SWEEP_CAP (a test hook) */
};

typedef struct cpr_mdp_pe {
  int64_t E;                  /* evaluations, >= 1 */
  const int32_t* point;       /* [E] index into the P probability arrays */
  const int32_t* policy;      /* [E][S] the action slot played, negative: none (a leaf) */
  int32_t states;             /* enum cpr_mdp_pe_states */
  int32_t n_start;            /* start states per evaluation (REACHABLE: >= 1; ALL: unused) */
  const int32_t* start_state; /* [E][n_start] */
  const double* start_prob;   /* [E][n_start] a start state counts if its probability is > 0 */
} cpr_mdp_pe;

typedef struct cpr_mdp_pe_opts {
  double theta;     /* >= 0 */
  double discount;  /* in (0, 1] */
  int64_t max_iter; /* >= 0; 0: until delta < theta (then theta must be > 0) */
  int32_t path;     /* enum cpr_mdp_vi_path; AUTO: resident if the states fit one workgroup and
                       its estimated sweep time is the lower one */
} cpr_mdp_pe_opts;
/* theta 1e-6, discount 1, max_iter 0, path AUTO */
int cpr_mdp_pe_opts_default(cpr_mdp_pe_opts* opts);

typedef struct cpr_mdp_pe_result {
  double* reward;    /* [E][S] */
  double* progress;  /* [E][S] */
  int64_t* iter;     /* [E] sweeps done */
  double* delta;     /* [E] max |reward - previous reward| of the last sweep */
  int32_t* status;   /* [E] enum cpr_mdp_pe_status */
  int32_t path_used; /* CPR_MDP_VI_RESIDENT or CPR_MDP_VI_GLOBAL */
  double kernel_ms;  /* HIP events around the launches, the status reads between them included */
} cpr_mdp_pe_result;

/* Per evaluation: the included states are found on the host before anything is launched (from
 * the start states with probability > 0 along the policy's used slots whose probability at the
 * evaluation's point is not exactly 0; a state with a negative policy entry is a leaf), or are
 * all states. reward = progress = 0; sweep i computes, for every included state with a policy
 * entry >= 0, r += prb (rew + discount reward[dst]) and p likewise over the used slots of that
 * action in slot order (f64, one rounding per operation); every other state stays 0. The
 * evaluation stops after sweep i if delta < theta (strict, unlike value iteration), else if
 * max_iter > 0 and i >= max_iter; evaluations stop independently. Every array of `result` is
 * filled. Checked before anything is launched (CPR_E_INVALID_ARG): what cpr_mdp_value_iteration
 * checks of `mdp`, E < 1, NULL arrays, a point outside [0, P), a policy entry >= A or one that
 * names an action with valid == 0 (at any state, reached or not), states REACHABLE with
 * n_start < 1 or a start state outside [0, S), an unknown `states`, discount outside (0, 1],
 * theta < 0, max_iter < 0, theta == 0 with max_iter == 0, an unknown path. CPR_E_CAPACITY: as
 * for value iteration. */
int cpr_mdp_policy_evaluation(cpr_ctx* ctx, const cpr_mdp* mdp, const cpr_mdp_pe* job,
                              const cpr_mdp_pe_opts* opts, cpr_mdp_pe_result* result);

#ifdef __cplusplus
}
#endif

#endif /* CPR_HIP_H */
