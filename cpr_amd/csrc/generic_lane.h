// One GPU lane = one episode of the reference's generic release/consider environment over
// Nakamoto consensus: gym/rust/src/generic/mod.rs Env (GenericEnv) with proto/nakamoto.rs,
// registered as Nakamoto-v0. The attacker acts per block on
// an explicit block DAG with the two primitive freedoms, withhold and ignore:
//   Release i   hand the i-th releasable block to the network           (mod.rs:683-693)
//   Consider i  let the attacker's own node see the i-th ignored block  (mod.rs:665-681)
//   Continue    communicate, then mine the next block                   (mod.rs:715-725)
// Episodes end by a Bernoulli(1/horizon) draw per unit of progress on the defenders' chain
// (mod.rs:789-793); on termination all withheld information is forced out (shutdown,
// mod.rs:728-758) and the defenders' chain is tracked a second time.
//
// State. Every block has a parent, a height and three views (mod.rs:21-43): AView Ignored /
// Considered / AEntry, DView Unknown / Known / DEntry, NView Honest / Withheld / Released. The
// lane keeps the two entry points in its header (GenericLane::aentry, ::dentry) instead of in a
// view value, so a block's view byte holds Ignored / Considered, Unknown / Known and the NView.
// Nakamoto blocks have one parent, and a block gets at most one honest and at most one attacker
// child (a miner's entry point moves to a higher block as soon as its child is seen and never
// comes back), so the children are two indices per block (hchild, achild; 0 = none, genesis is
// nobody's child).
//
// Action lists (available_actions, mod.rs:286-314) in the reference's order, increasing block
// index, kept incrementally: a block enters `rel` when it is mined withheld on a parent that is
// not withheld, or when its withheld parent is released; it enters `con` when it is mined
// ignored on a parent that is not ignored, or when its ignored parent is considered. Both by
// sorted insertion. `pend` is just_released (mod.rs:695-703), blocks released but not yet
// delivered, in the same order. The defender block on the wire (just_mined_by_defender,
// mod.rs:705-713) is at most one: GenericLane::wire.
//
// Randomness from the keyed stream, tag TAG_GENERIC, step index j:
//   Continue at step j   block(j, TAG_GENERIC): w1 < t_gamma the attacker communicates fast
//                        (communicate, mod.rs:795-819), then w0 < t_alpha the attacker mines
//   shutdown at step j   w2 < t_gamma of the same block: fast in shutdown (mod.rs:751)
//   termination unit i   word i & 3 of block(j, TAG_GENERIC | 0x100000 | i >> 2) < t_term, one
//                        per unit of the step's progress before shutdown; fires if any fires,
//                        the law of the reference's 1 - (1 - 1/H)^progress (mod.rs:789-793)
// A step that is not Continue draws nothing but its termination words (its progress is 0, so
// none). Thresholds are floor(p * 2^32) and each draw is an integer compare; the reference
// compares x <= p on an f32 uniform, a measure-zero difference accepted as for FC16.
//
// Host-compilable: tests/native_generic replays command files through these functions against
// tests/generic_env_ref.py. The lane never reads a byte of its block storage that it did not
// write in the same episode (the pool holds what the previous launch left).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "cpr_stream.h"

namespace cpr {
namespace generic {

constexpr uint32_t TAG_GENERIC = 0xB0000000u;
// cfg.max_steps above this is refused; the reference registers Nakamoto-v0 with
// max_episode_steps = 1000. Block indices are uint16_t.
constexpr int32_t kGenericMaxSteps = 4096;
constexpr int32_t kGenericMaxK = 11;  // 1 + 2K head actions <= kPolMaxActions (24)
constexpr uint32_t kStCapacity = 32u;        // CPR_ST_CAPACITY
constexpr uint32_t kStReferenceRaises = 64u;  // CPR_ST_REFERENCE_RAISES

// view byte of a block
enum : uint8_t {
  AV_CONSIDERED = 1u,  // else Ignored
  DV_KNOWN = 2u,       // else Unknown
  NV_WITHHELD = 4u,    // neither: Honest
  NV_RELEASED = 8u,
};

struct GenericParams {
  uint64_t t_alpha, t_gamma, t_term;  // floor(p * 2^32)
  int32_t max_steps;                  // truncation cap; the lane holds max_steps + 1 blocks
};

// The lane's block storage: cap = max_steps + 1 entries per array
struct GenericBlocks {
  uint16_t *parent, *height, *hchild, *achild;  // per block
  uint16_t *rel, *con, *pend;                   // the three sorted lists
  uint8_t* view;                                // per block
};

constexpr int32_t kGenericBytesPerBlock = 7 * 2 + 1;

__host__ __device__ inline size_t generic_region_bytes(int32_t max_steps) {
  const size_t b = (size_t)(max_steps + 1) * kGenericBytesPerBlock;
  return (b + 127) / 128 * 128;  // whole 128-byte lines per lane
}

__host__ __device__ inline GenericBlocks generic_blocks(void* region, int32_t max_steps) {
  const size_t cap = (size_t)max_steps + 1;
  uint16_t* p = (uint16_t*)region;
  GenericBlocks B;
  B.parent = p;
  B.height = p + cap;
  B.hchild = p + 2 * cap;
  B.achild = p + 3 * cap;
  B.rel = p + 4 * cap;
  B.con = p + 5 * cap;
  B.pend = p + 6 * cap;
  B.view = (uint8_t*)(p + 7 * cap);
  return B;
}

// The fixed-size part of a lane, read and written as a unit; one 128-byte line
struct alignas(128) GenericLane {
  uint64_t ep;
  int64_t era, erd, eprog, rewrites;  // episode sums (mod.rs:542-548 summed over the steps)
  int32_t n_blocks, aentry, dentry;
  int32_t hist;  // tip of the defenders' chain at the last track_defender_chain (Env::hist)
  int32_t ca;    // cached common ancestor (Env::ca)
  int32_t n_rel, n_con, n_pend;
  int32_t wire;  // the defender block mined but not delivered, or -1
  int32_t mined, steps, last_rewrite;
  uint32_t status;
  int32_t live;  // 0 never reset, 1 running, 2 over (steps are ignored until the next reset)
};

struct GenericStep {
  int32_t reward_attacker, reward_defender, progress, rewrite, time;
  bool terminated;
};

// ---------------------------------------------------------------- actions (mod.rs:214-279)
// integer form: 0 Continue, -(i + 1) Release(i), +(i + 1) Consider(i), i <= 255

__host__ __device__ inline int32_t generic_clamp_action(int32_t a) {
  return a < -256 ? -256 : (a > 256 ? 256 : a);
}

// encode_action (mod.rs:236-248) of the integer form, f32 with IEEE division
__host__ __device__ inline float generic_encode_action(int32_t a) {
  if (a == 0) return 0.f;
  const float x = (float)generic_clamp_action(a);
  return x / (1.f + __builtin_fabsf(x));
}

// decode_action (mod.rs:250-279): false where the reference asserts (outside [-1, 1], NaN)
__host__ __device__ inline bool generic_decode_action(float a, int32_t* out) {
  if (!(a >= -1.f) || !(a <= 1.f)) return false;
  if (a == -1.f) { *out = -256; return true; }
  if (a == 1.f) { *out = 256; return true; }
  float x = a >= 0.f ? -a / (a - 1.f) : a / (a + 1.f);
  x = __builtin_roundf(x);  // f32::round: half away from zero
  if (x < -256.f)
    *out = -256;
  else if (x < 0.f)
    *out = -((int32_t)(-x - 1.f) + 1);
  else if (x > 256.f)
    *out = 256;
  else if (x > 0.f)
    *out = (int32_t)(x - 1.f) + 1;
  else
    *out = 0;
  return true;
}

// The categorical head of 1 + 2K actions: 0 Continue, 1 .. K Release(0 .. K-1),
// K+1 .. 2K Consider(0 .. K-1), to the integer form
__host__ __device__ inline int32_t generic_head_action(int32_t index, int32_t k) {
  if (index <= 0 || index > 2 * k) return 0;
  return index <= k ? -index : index - k;
}

// ---------------------------------------------------------------- the lists

__host__ __device__ inline void list_insert(uint16_t* l, int32_t& n, int32_t b) {
  int32_t i = n;
  while (i > 0 && (int32_t)l[i - 1] > b) {
    l[i] = l[i - 1];
    --i;
  }
  l[i] = (uint16_t)b;
  ++n;
}

__host__ __device__ inline void list_remove_at(uint16_t* l, int32_t& n, int32_t i) {
  for (int32_t q = i; q + 1 < n; ++q) l[q] = l[q + 1];
  --n;
}

// ---------------------------------------------------------------- the env

__host__ __device__ inline void generic_start(const GenericBlocks& B, GenericLane& L,
                                              uint64_t ep) {
  // init_graph (mod.rs:340-351): genesis is both entry points, Honest, height 0
  B.parent[0] = 0;
  B.height[0] = 0;
  B.hchild[0] = 0;
  B.achild[0] = 0;
  B.view[0] = AV_CONSIDERED | DV_KNOWN;
  L.ep = ep;
  L.era = L.erd = L.eprog = L.rewrites = 0;
  L.n_blocks = 1;
  L.aentry = L.dentry = L.hist = L.ca = 0;
  L.n_rel = L.n_con = L.n_pend = 0;
  L.wire = -1;
  L.mined = L.steps = L.last_rewrite = 0;
  L.status = 0u;
  L.live = 1;
}

// deliver (mod.rs:647-663) with nakamoto.rs:27-33 update: the defenders prefer b if it is
// strictly higher
__host__ __device__ inline void generic_deliver(const GenericBlocks& B, GenericLane& L,
                                                int32_t b) {
  // mod.rs:648-654: repeated delivery / missing dependencies
  if ((B.view[b] & DV_KNOWN) || !(B.view[B.parent[b]] & DV_KNOWN)) L.status |= kStReferenceRaises;
  B.view[b] |= DV_KNOWN;
  if (B.height[b] > B.height[L.dentry]) L.dentry = b;
}

// consider (mod.rs:665-681). The reference builds the view it hands to update with
// defender_view, not the attacker's (mod.rs:678); Nakamoto's update reads heights only
// (nakamoto.rs:27-33), so the view has no effect and none is built here.
__host__ __device__ inline void generic_consider(const GenericBlocks& B, GenericLane& L,
                                                 int32_t b) {
  // mod.rs:666-672: repeated consider / missing dependencies
  if ((B.view[b] & AV_CONSIDERED) || !(B.view[B.parent[b]] & AV_CONSIDERED))
    L.status |= kStReferenceRaises;
  B.view[b] |= AV_CONSIDERED;
  if (B.height[b] > B.height[L.aentry]) L.aentry = b;
}

// release (mod.rs:683-693)
__host__ __device__ inline void generic_release(const GenericBlocks& B, GenericLane& L,
                                                int32_t b) {
  // mod.rs:684-690: unsuitable block / missing dependencies
  if (!(B.view[b] & NV_WITHHELD) || (B.view[B.parent[b]] & NV_WITHHELD))
    L.status |= kStReferenceRaises;
  B.view[b] = (uint8_t)((B.view[b] & ~NV_WITHHELD) | NV_RELEASED);
}

__host__ __device__ inline int32_t generic_add_block(const GenericBlocks& B, GenericLane& L,
                                                     int32_t parent, uint8_t view) {
  const int32_t b = L.n_blocks;
  B.parent[b] = (uint16_t)parent;
  B.height[b] = (uint16_t)(B.height[parent] + 1);  // nakamoto.rs:19-25
  B.hchild[b] = 0;
  B.achild[b] = 0;
  B.view[b] = view;
  L.n_blocks = b + 1;
  L.mined += 1;
  return b;
}

// continue_ (mod.rs:715-725): communicate (mod.rs:795-819), then the miner draw
__host__ __device__ inline void generic_continue(const GenericParams& P, const GenericBlocks& B,
                                                 GenericLane& L, const Words4& w) {
  const bool fast = (uint64_t)w.w1 < P.t_gamma;
  if (!fast && L.wire >= 0) generic_deliver(B, L, L.wire);
  for (int32_t q = 0; q < L.n_pend; ++q) generic_deliver(B, L, B.pend[q]);
  if (fast && L.wire >= 0) generic_deliver(B, L, L.wire);
  L.n_pend = 0;
  L.wire = -1;
  if ((uint64_t)w.w0 < P.t_alpha) {
    // mine_attacker (mod.rs:837-852) on the attacker's entry, considered at once (mod.rs:719-721)
    const int32_t p = L.aentry;
    const int32_t b = generic_add_block(B, L, p, NV_WITHHELD);
    B.achild[p] = (uint16_t)b;
    generic_consider(B, L, b);
    if (!(B.view[p] & NV_WITHHELD)) B.rel[L.n_rel++] = (uint16_t)b;  // the highest index
  } else {
    // mine_defender (mod.rs:821-835) on the defenders' entry: Ignored, Unknown, Honest
    const int32_t p = L.dentry;
    const int32_t b = generic_add_block(B, L, p, 0u);
    B.hchild[p] = (uint16_t)b;
    L.wire = b;
    if (B.view[p] & AV_CONSIDERED) B.con[L.n_con++] = (uint16_t)b;
  }
}

// shutdown (mod.rs:728-758): every withheld block is released and delivered, in block order,
// before or after the defender block on the wire. The action lists stay as they were: the
// reference does not recompute them after shutdown, and the last observation shows them.
template <class Wire>
__host__ __device__ inline void generic_shutdown(const GenericParams& P, const GenericBlocks& B,
                                                 GenericLane& L, const Words4& w, Wire&& seen) {
  const bool fast = (uint64_t)w.w2 < P.t_gamma;
  seen(fast, L.wire >= 0);
  // mod.rs:748 (at most one defender block on the wire) holds by construction: wire is one index
  if (!fast && L.wire >= 0) generic_deliver(B, L, L.wire);
  for (int32_t b = 0; b < L.n_blocks; ++b)
    if (B.view[b] & NV_WITHHELD) {
      generic_release(B, L, b);
      generic_deliver(B, L, b);
    }
  if (fast && L.wire >= 0) generic_deliver(B, L, L.wire);
  L.wire = -1;
}

// track_defender_chain (mod.rs:557-623): what the defenders' chain gained and dropped since
// the last call, by walking parent pointers from the new and the old tip to their fork point
__host__ __device__ inline void generic_track(const GenericBlocks& B, GenericLane& L,
                                              GenericStep& t) {
  int32_t c = L.dentry, o = L.hist;  // nakamoto.rs:35-37: the tip is the entry point
  if (c == o) return;
  if (B.height[c] < B.height[o]) L.status |= kStReferenceRaises;  // mod.rs:578
  int32_t prg = 0, ra = 0, rd = 0, upd = 0;
  auto gain = [&](int32_t b, int32_t s) {  // nakamoto.rs:48-54: progress 1, reward 1 to the miner
    prg += s;
    if (B.view[b] & (NV_WITHHELD | NV_RELEASED))
      ra += s;
    else
      rd += s;
  };
  while (B.height[c] > B.height[o]) {
    gain(c, 1);
    c = B.parent[c];
  }
  while (B.height[o] > B.height[c]) {  // only after mod.rs:578 would have raised
    gain(o, -1);
    ++upd;
    o = B.parent[o];
  }
  while (c != o) {
    gain(c, 1);
    gain(o, -1);
    ++upd;
    c = B.parent[c];
    o = B.parent[o];
  }
  L.hist = L.dentry;
  if (prg < 0) L.status |= kStReferenceRaises;  // mod.rs:499
  t.progress += prg;
  t.reward_attacker += ra;
  t.reward_defender += rd;
  t.rewrite += upd;
}

// common_history's last block (mod.rs:864-882): the fork point of the two entry points
__host__ __device__ inline int32_t generic_common_ancestor(const GenericBlocks& B, int32_t a,
                                                           int32_t d) {
  while (B.height[a] > B.height[d]) a = B.parent[a];
  while (B.height[d] > B.height[a]) d = B.parent[d];
  while (a != d) {
    a = B.parent[a];
    d = B.parent[d];
  }
  return a;
}

// One step with the integer action (mod.rs:446-555). `seen(fast, wire)` is called once if the
// step runs shutdown, with its coin and whether a defender block was on the wire (the host
// fuzz's coverage).
template <class St, class Wire>
__host__ __device__ inline GenericStep generic_step(const GenericParams& P, const St& S,
                                                    const GenericBlocks& B, GenericLane& L,
                                                    int32_t action, Wire&& seen) {
  GenericStep t{0, 0, 0, 0, 0, false};
  const uint32_t j = (uint32_t)L.steps;
  const int32_t a0 = L.aentry, d0 = L.dentry;
  // guarded_action (mod.rs:418-444): past the list acts as its last entry, an empty list as
  // Continue
  action = generic_clamp_action(action);
  int32_t i = action < 0 ? -action - 1 : action - 1;
  const int32_t l = action < 0 ? L.n_rel : L.n_con;
  if (action != 0 && l < 1) action = 0;
  if (action != 0 && i >= l) i = l - 1;
  Words4 w{0u, 0u, 0u, 0u};
  if (action < 0) {
    const int32_t b = B.rel[i];
    generic_release(B, L, b);
    list_remove_at(B.rel, L.n_rel, i);
    if (B.achild[b]) list_insert(B.rel, L.n_rel, B.achild[b]);  // withheld as its parent was
    list_insert(B.pend, L.n_pend, b);
  } else if (action > 0) {
    const int32_t b = B.con[i];
    generic_consider(B, L, b);
    list_remove_at(B.con, L.n_con, i);
    if (B.hchild[b]) list_insert(B.con, L.n_con, B.hchild[b]);  // ignored as its parent was
  } else if (L.n_blocks <= P.max_steps) {  // always: one block per Continue, steps < max_steps
    w = S.block(j, TAG_GENERIC);
    generic_continue(P, B, L, w);
    t.time = 1;
  } else {
    L.status |= kStCapacity;
  }
  // the cached common ancestor (mod.rs:472-473). An entry point that moved to its own child
  // while it was not the common ancestor leaves the fork point where it is; anything else
  // walks.
  const bool a_same = L.aentry == a0 || (B.parent[L.aentry] == a0 && a0 != L.ca);
  const bool d_same = L.dentry == d0 || (B.parent[L.dentry] == d0 && d0 != L.ca);
  if (!(a_same && d_same)) L.ca = generic_common_ancestor(B, L.aentry, L.dentry);
  generic_track(B, L, t);
  // env_terminates (mod.rs:789-793) on the progress before shutdown
  for (int32_t u = 0; u < t.progress && !t.terminated; u += 4) {
    const Words4 x = S.block(j, TAG_GENERIC | 0x100000u | (uint32_t)(u >> 2));
    const uint32_t xw[4] = {x.w0, x.w1, x.w2, x.w3};
    for (int32_t q = 0; q < 4 && u + q < t.progress; ++q)
      t.terminated |= (uint64_t)xw[q] < P.t_term;
  }
  if (t.terminated) {  // mod.rs:519-537; progress > 0, so this step was a Continue and w is drawn
    generic_shutdown(P, B, L, w, seen);
    generic_track(B, L, t);
  }
  L.steps += 1;
  L.era += t.reward_attacker;
  L.erd += t.reward_defender;
  L.eprog += t.progress;
  L.rewrites += t.rewrite;
  L.last_rewrite = t.rewrite;
  return t;
}

template <class St>
__host__ __device__ inline GenericStep generic_step(const GenericParams& P, const St& S,
                                                    const GenericBlocks& B, GenericLane& L,
                                                    int32_t action) {
  return generic_step(P, S, B, L, action, [](bool, bool) {});
}

// The step of the lockstep env: the episode is over at termination, or after max_steps steps
// without one (CPR_ST_CAPACITY, as CPR_PROTO_FC16_ENV truncates; the reference leaves that to
// gymnasium's TimeLimit and runs no shutdown then). A lane whose episode is over ignores
// further steps until its reset (all-zero step, done), which is what bounds the DAG by
// max_steps + 1 blocks.
template <class St, class Wire>
__host__ __device__ inline bool generic_env_step(const GenericParams& P, const St& S,
                                                 const GenericBlocks& B, GenericLane& L,
                                                 int32_t action, GenericStep* t, Wire&& seen) {
  if (L.live != 1) {
    *t = GenericStep{0, 0, 0, 0, 0, false};
    return true;
  }
  *t = generic_step(P, S, B, L, action, seen);
  bool done = t->terminated;
  if (!done && L.steps >= P.max_steps) {
    L.status |= kStCapacity;
    done = true;
  }
  if (done) L.live = 2;
  return done;
}

// The observation (mod.rs:884-911, nakamoto.rs:71-104) as the reference's five f32:
// a - ca, d - ca (with the fresh defender child of the defenders' entry), match feasible,
// encode(Release(n_release - 1)) or 0, encode(Consider(n_consider - 1)) or 0. The reference
// casts n - 1 to u8, so a list of more than 256 wraps; restated as written.
struct GenericObs {
  int32_t a, d, mf;
};

__host__ __device__ inline GenericObs generic_observe_fields(const GenericBlocks& B,
                                                             GenericLane& L) {
  const int32_t ch = B.height[L.ca];
  GenericObs o{B.height[L.aentry] - ch, B.height[L.dentry] - ch, 0};
  const int32_t c = B.hchild[L.dentry];  // children(def) mined by a defender: at most one
  if (c) {
    // nakamoto.rs:94-98: the child is a leaf, unknown to the defenders, one higher
    if (B.hchild[c] || B.achild[c] || (B.view[c] & DV_KNOWN)) L.status |= kStReferenceRaises;
    o.d += 1;
    o.mf = 1;
  }
  return o;
}

__host__ __device__ inline void generic_observe(const GenericBlocks& B, GenericLane& L,
                                                float* o) {
  const GenericObs f = generic_observe_fields(B, L);
  o[0] = (float)f.a;
  o[1] = (float)f.d;
  o[2] = (float)f.mf;
  o[3] = L.n_rel > 0 ? generic_encode_action(-(((L.n_rel - 1) & 255) + 1)) : 0.f;
  o[4] = L.n_con > 0 ? generic_encode_action(((L.n_con - 1) & 255) + 1) : 0.f;
}

}  // namespace generic
}  // namespace cpr
