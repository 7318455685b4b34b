"""Table policies for the device's table-driven Nakamoto path from the selfish-mining MDP.

SURVEY.md §8f rank 4: the reference derives optimal withholding policies offline with its
MDP toolbox — the Sapirshtein et al. (FC'16) Bitcoin model (`mdp/lib/models/fc16sapirshtein.py:
21-205`), explored breadth-first into an explicit MDP (`mdp/lib/compiler.py:6-90`), mapped to
a probabilistically terminating MDP (`mdp/lib/models/aft20barzur.py:244-300` `ptmdp`) and
solved by value iteration (`mdp/lib/explicit_mdp.py:97-177`, used as in
`mdp/sprint-0-explicit-mdps/util.py:6-14`). This module restates that pipeline (same state
order, same transition order, same floating-point accumulation order, same first-best
tie rule) and turns the policy into the `dim * dim * 2` action table that `CPR_POLICY_TABLE`
evaluates on the device (`nakamoto_lane.h` `nak_policy`: index `(h * dim + a) * 2 + event`).

Host-side numpy; nothing here runs per step. The value iteration also runs on the device
(`value_iteration_device`, `solve_grid`: every point of an alpha x gamma grid in one call).
"""

from collections import deque

import numpy as np

# fc16sapirshtein.py:11-19 (same encoding as nakamoto_ssz's Action ranks)
ADOPT, OVERRIDE, MATCH, WAIT = 0, 1, 2, 3
IRRELEVANT, RELEVANT, ACTIVE = 0, 1, 2


class BitcoinSM:
    """fc16sapirshtein.BitcoinSM: states (a, h, fork), actions per state in the model's
    order, transitions as (state, probability, reward, progress)."""

    def __init__(self, alpha, gamma, maximum_fork_length, maximum_dag_size=0):
        if alpha < 0 or alpha >= 0.5:
            raise ValueError("alpha must be between 0 and 0.5")
        if gamma < 0 or gamma > 1:
            raise ValueError("gamma must be between 0 and 1")
        self.alpha, self.gamma = alpha, gamma
        self.mfl, self.mds = maximum_fork_length, maximum_dag_size

    def start(self):  # :60-64
        return [((1, 0, IRRELEVANT), self.alpha), ((0, 1, IRRELEVANT), 1 - self.alpha)]

    def truncated(self, s):  # :66-77
        a, h, _ = s
        if self.mfl > 0 and (a >= self.mfl or h >= self.mfl):
            return True
        return self.mds > 0 and a + h + 1 >= self.mds

    def actions(self, s):  # :79-91
        a, h, fork = s
        acts = []
        if not self.truncated(s):
            acts.append(WAIT)
        if a > h:
            acts.append(OVERRIDE)
        if a >= h and fork == RELEVANT:
            acts.append(MATCH)
        acts.append(ADOPT)
        return acts

    def apply(self, act, s):  # :93-183
        a, h, fork = s
        al, ga = self.alpha, self.gamma
        if act == ADOPT:
            return [((1, 0, IRRELEVANT), al, 0, h), ((0, 1, IRRELEVANT), 1 - al, 0, h)]
        if act == OVERRIDE:
            return [((a - h, 0, IRRELEVANT), al, h + 1, h + 1),
                    ((a - h - 1, 1, RELEVANT), 1 - al, h + 1, h + 1)]
        if act == WAIT and fork != ACTIVE:
            return [((a + 1, h, IRRELEVANT), al, 0, 0.0), ((a, h + 1, RELEVANT), 1 - al, 0, 0)]
        # MATCH, or WAIT while a match is active
        return [((a + 1, h, ACTIVE), al, 0, 0.0),
                ((a - h, 1, RELEVANT), ga * (1 - al), h, h),
                ((a, h + 1, RELEVANT), (1 - ga) * (1 - al), 0, 0)]


def compile_mdp(model):
    """compiler.py:6-90: breadth-first exploration; state ids in discovery order, action ids
    = positions in model.actions(state). Returns (states, tab) with
    tab[s][i] = [(dst, p, reward, progress), ...]."""
    ids, states, tab = {}, [], []
    queue, explored = deque(), set()
    for s, _p in model.start():
        ids[s] = len(states)
        states.append(s)
        tab.append([])
        queue.append(s)
    while queue:
        s = queue.popleft()
        if s in explored:
            continue
        explored.add(s)
        sid = ids[s]
        for act in model.actions(s):
            lst = []
            for to, p, r, prg in model.apply(act, s):
                if to not in ids:
                    ids[to] = len(states)
                    states.append(to)
                    tab.append([])
                    queue.append(to)
                lst.append((ids[to], p, r, prg))
            tab[sid].append(lst)
    return states, tab


def ptmdp(tab, horizon):
    """aft20barzur.py:244-300: one terminal state (the last id); every transition with
    progress > 0 splits into termination with 1 - (1 - 1/H)^progress and the rest."""
    assert horizon > 0
    terminal = len(tab)
    out = []
    for actions in tab:
        new_actions = []
        for lst in actions:
            nl = []
            for dst, p, r, prg in lst:
                if prg == 0.0:
                    nl.append((dst, p, r, prg))
                else:
                    term = 1.0 - ((1.0 - (1.0 / horizon)) ** prg)
                    nl.append((terminal, term * p, 0.0, 0.0))
                    nl.append((dst, (1 - term) * p, r, prg))
            new_actions.append(nl)
        out.append(new_actions)
    out.append([])  # the terminal state has no actions
    return out


def pack(tab):
    """The dense padded arrays of ``tab`` (compile_mdp / ptmdp form) that both solvers read:
    dst, prb, rew, prg, used [S][A][T] and valid [S][A], A and T the largest action and
    transition counts; padding slots hold zeros and used = False."""
    n = len(tab)
    n_act = max((len(a) for a in tab), default=0)
    n_tr = max((len(l) for a in tab for l in a), default=0)
    dst = np.zeros((n, n_act, n_tr), np.int64)
    prb = np.zeros((n, n_act, n_tr))
    rew = np.zeros((n, n_act, n_tr))
    prg = np.zeros((n, n_act, n_tr))
    valid = np.zeros((n, n_act), bool)
    used = np.zeros((n, n_act, n_tr), bool)
    for s, actions in enumerate(tab):
        for i, lst in enumerate(actions):
            valid[s, i] = True
            for j, (d, p, r, g) in enumerate(lst):
                dst[s, i, j], prb[s, i, j], rew[s, i, j], prg[s, i, j] = d, p, r, g
                used[s, i, j] = True
    return dict(dst=dst, prb=prb, rew=rew, prg=prg, valid=valid, used=used)


_PACK_KEYS = ("dst", "prb", "rew", "prg", "valid", "used")


def _packed(tab):
    """``tab`` packed, or itself if it is a packed MDP already (a dict of pack's arrays)."""
    if isinstance(tab, dict):
        missing = [k for k in _PACK_KEYS if k not in tab]
        if missing:
            raise ValueError(f"packed MDP without {missing}")
        return tab
    return pack(tab)


def value_iteration(tab, *, stop_delta, discount=1.0, max_iter=0):
    """explicit_mdp.py:97-177 vectorised over states: per (state, action) the transitions
    accumulate in their order, the first action with the strictly best value wins. ``tab`` may
    be a packed MDP (``pack``); whatever its padding slots hold is ignored."""
    m = _packed(tab)
    used = np.asarray(m["used"], bool)
    valid = np.asarray(m["valid"], bool)
    dst = np.where(used, m["dst"], 0)
    prb = np.where(used, m["prb"], 0.0)
    rew = np.where(used, m["rew"], 0.0)
    prg = np.where(used, m["prg"], 0.0)
    n, n_act, n_tr = dst.shape
    value = np.zeros(n)
    progress = np.zeros(n)
    policy = np.zeros(n, np.int64)
    it = 1
    while True:
        this_v = np.zeros((n, n_act))
        this_p = np.zeros((n, n_act))
        for j in range(n_tr):  # += in transition order, as the reference's inner loop
            tv = prb[:, :, j] * (rew[:, :, j] + discount * value[dst[:, :, j]])
            tp = prb[:, :, j] * (prg[:, :, j] + discount * progress[dst[:, :, j]])
            this_v = np.where(used[:, :, j], this_v + tv, this_v)
            this_p = np.where(used[:, :, j], this_p + tp, this_p)
        best_a = np.full(n, -1, np.int64)
        best_v = np.zeros(n)
        best_p = np.zeros(n)
        for i in range(n_act):  # `this_v > best_v or best_a < 0`
            take = valid[:, i] & ((this_v[:, i] > best_v) | (best_a < 0))
            best_a = np.where(take, i, best_a)
            best_v = np.where(take, this_v[:, i], best_v)
            best_p = np.where(take, this_p[:, i], best_p)
        delta = float(np.abs(best_v - value).max()) if n else 0.0
        value, progress, policy = best_v, best_p, best_a
        if max_iter > 0 and it >= max_iter:
            break
        if delta <= stop_delta:
            break
        it += 1
    return dict(vi_policy=policy, vi_value=value, vi_progress=progress, vi_iter=it,
                vi_delta=delta)


def value_iteration_device(tabs, *, stop_delta, discount=1.0, max_iter=0, path="auto", ctx=None):
    """``value_iteration`` on the device (``device.Context.mdp_value_iteration``) for one MDP
    or a list of MDPs that share a topology (everything but the probabilities; ``tab``s or
    packed MDPs), all solved in one call. Returns one dict per MDP (a single dict for a single
    MDP) with the host solver's keys, bit for bit its results, plus ``vi_status`` (0 converged,
    1 stopped at max_iter, 2 not converged at the library's sweep cap), ``vi_path`` and
    ``vi_kernel_ms`` (the whole call's)."""
    from . import device

    single, ms = _one_topology(tabs)
    first = ms[0]
    used = np.asarray(first["used"], bool)
    ctx = ctx or device.default_context()
    r = ctx.mdp_value_iteration(first["dst"], used, first["valid"], first["rew"], first["prg"],
                                np.stack([np.asarray(m["prb"], np.float64) for m in ms]),
                                stop_delta=stop_delta, discount=discount, max_iter=max_iter,
                                path=path)
    out = [dict(vi_policy=r["policy"][p].astype(np.int64), vi_value=r["value"][p],
                vi_progress=r["progress"][p], vi_iter=int(r["iter"][p]),
                vi_delta=float(r["delta"][p]), vi_status=int(r["status"][p]),
                vi_path=r["path_used"], vi_kernel_ms=r["kernel_ms"])
           for p in range(len(ms))]
    return out[0] if single else out


def _one_topology(tabs):
    """(single, packed MDPs) of one MDP or a list of MDPs, which must share a topology."""
    single = _is_single(tabs)
    ms = [_packed(tabs)] if single else [_packed(t) for t in tabs]
    if not ms:
        raise ValueError("no MDP to solve")
    first = ms[0]
    used = np.asarray(first["used"], bool)
    for m in ms[1:]:
        if np.shape(m["dst"]) != np.shape(first["dst"]) \
                or not np.array_equal(np.asarray(m["used"], bool), used) \
                or not np.array_equal(np.asarray(m["valid"], bool),
                                      np.asarray(first["valid"], bool)) \
                or any(not np.array_equal(np.where(used, m[k], 0), np.where(used, first[k], 0))
                       for k in ("dst", "rew", "prg")):
            raise ValueError("the MDPs do not share one topology (states, actions, "
                             "destinations, rewards and progress must agree)")
    if np.asarray(first["dst"]).size == 0:
        raise ValueError("an MDP needs at least one state, action slot and transition slot")
    return single, ms


# ---- policy evaluation (explicit_mdp.py:179-208, 328-378)

def _checked_policy(m, policy):
    """``policy`` as an int64 array over the states of the packed MDP ``m``; an entry >= 0 must
    name an action slot its state offers (the reference raises IndexError only where it
    happens to reach such a state; here it is a ValueError wherever it stands)."""
    valid = np.asarray(m["valid"], bool)
    n, n_act = valid.shape
    policy = np.asarray(policy)
    if policy.shape != (n,) or policy.dtype.kind not in "iu":
        raise ValueError(f"policy: expected {n} integers, one action slot (or -1) per state")
    policy = policy.astype(np.int64)
    bad = policy >= n_act
    ok = (policy >= 0) & ~bad
    bad[ok] = ~valid[np.nonzero(ok)[0], policy[ok]]
    if bad.any():
        s = int(np.nonzero(bad)[0][0])
        raise ValueError(f"policy: state {s} does not offer action slot {int(policy[s])}")
    return policy


def _checked_start(start, n):
    if start is None:  # compile_mdp numbers model.start() 0 and 1
        start = [(s, 1.0) for s in range(min(2, n))]
    start = [(int(s), float(p)) for s, p in start]
    if not start:
        raise ValueError("start: expected at least one (state id, probability)")
    for s, _p in start:
        if not 0 <= s < n:
            raise ValueError(f"start: state {s} is outside [0, {n})")
    return start


def reachable_states(tab, policy, start=None):
    """explicit_mdp.py:179-208: the set of states that ``policy`` reaches from the start states
    with probability > 0 (``start``: a list of (state id, probability); default ids 0 and 1, as
    ``compile_mdp`` numbers ``model.start()``, both counted), following ``tab[s][policy[s]]``.
    Transitions with probability exactly 0 are skipped; a state with ``policy[s] < 0`` is a
    leaf. ``tab`` may be a packed MDP."""
    m = _packed(tab)
    policy = _checked_policy(m, policy)
    used = np.asarray(m["used"], bool)
    dst, prb = np.asarray(m["dst"]), np.asarray(m["prb"])
    todo = [s for s, p in _checked_start(start, len(policy)) if p > 0]
    reachable = set(todo)
    while todo:
        s = todo.pop()
        a = policy[s]
        if a < 0:
            continue
        for j in np.nonzero(used[s, a] & (prb[s, a] != 0.0))[0]:
            d = int(dst[s, a, j])
            if d not in reachable:
                reachable.add(d)
                todo.append(d)
    return reachable


def policy_evaluation(tab, policy, *, theta, discount=1.0, start=None, states="reachable",
                      max_iter=None):
    """explicit_mdp.py:328-378 vectorised over states, bit for bit its results. The included
    states are those ``reachable_states(tab, policy, start)`` gives (``states="reachable"``,
    the reference's ``around_state=None``) or all of them (``states="all"``, the reference's
    ``around_state`` given, whatever its value). Sweep i (from 1) computes, for every included
    state with ``policy[s] >= 0``, r += prb * (rew + discount * reward_prev[dst]) and p
    likewise over the transitions of ``tab[s][policy[s]]`` in their order (f64, one rounding
    per operation); every other state stays 0 in reward and progress. delta is the largest
    ``|new - old|`` of the reward vector over all states.

    The reference's quirks are kept: the run stops when ``delta < theta`` (strict, where value
    iteration stops at ``<=``), and only then asks whether ``max_iter`` is set and
    ``i >= max_iter``, so a run that converges in its last allowed sweep counts as converged
    and ``max_iter=0`` stops after the first sweep; a state outside the included set
    contributes 0 to its predecessors for ever, also with ``states="all"`` and a policy of -1.
    Unlike the reference, a ``policy[s]`` that names a slot its state does not offer is a
    ``ValueError`` (there: an IndexError, and only if the state is reached).

    Returns ``pe_reward``, ``pe_progress``, ``pe_iter`` and ``pe_delta``. ``tab`` may be a
    packed MDP, as for ``value_iteration``."""
    m = _packed(tab)
    policy = _checked_policy(m, policy)
    if states not in ("reachable", "all"):
        raise ValueError('states: expected "reachable" or "all"')
    if not theta >= 0:
        raise ValueError("theta must be >= 0")
    if theta == 0 and max_iter is None:
        raise ValueError("infinite iteration: theta == 0 and no max_iter")
    n = len(policy)
    included = np.ones(n, bool)
    if states == "reachable":
        included[:] = False
        included[list(reachable_states(m, policy, start))] = True
    act = included & (policy >= 0)
    rows, slot = np.arange(n), np.where(act, policy, 0)
    used = np.asarray(m["used"], bool)[rows, slot] & act[:, None]
    dst = np.where(used, np.asarray(m["dst"])[rows, slot], 0)
    prb = np.where(used, np.asarray(m["prb"], np.float64)[rows, slot], 0.0)
    rew = np.where(used, np.asarray(m["rew"], np.float64)[rows, slot], 0.0)
    prg = np.where(used, np.asarray(m["prg"], np.float64)[rows, slot], 0.0)
    reward = np.zeros(n)
    progress = np.zeros(n)
    i = 1
    while True:
        r = np.zeros(n)
        p = np.zeros(n)
        for j in range(dst.shape[1]):  # += in transition order, as the reference's inner loop
            tr = prb[:, j] * (rew[:, j] + discount * reward[dst[:, j]])
            tp = prb[:, j] * (prg[:, j] + discount * progress[dst[:, j]])
            r = np.where(used[:, j], r + tr, r)
            p = np.where(used[:, j], p + tp, p)
        delta = float(np.abs(r - reward).max()) if n else 0.0
        reward, progress = r, p
        if delta < theta:
            break
        if max_iter is not None and i >= max_iter:
            break
        i += 1
    return dict(pe_reward=reward, pe_progress=progress, pe_iter=i, pe_delta=delta)


def policy_evaluation_device(tabs, policies, pairs=None, *, theta, discount=1.0, start=None,
                             states="reachable", max_iter=None, path="auto", ctx=None):
    """``policy_evaluation`` on the device (``device.Context.mdp_policy_evaluation``) for
    Q policies x P points in one call. ``tabs``: one MDP or a list of MDPs that share a
    topology (as for ``value_iteration_device``), the points; ``policies``: [Q][S]; ``pairs``:
    a list of (policy index, point index), by default the full cross product, policy-major.
    ``start``: as for ``policy_evaluation``, one list for every evaluation or one list per
    point (the start probabilities of a model depend on its alpha). ``max_iter``: None or
    >= 1. Returns one dict per pair with the host's keys, bit for bit its results, plus
    ``pe_status`` (0 converged, 1 stopped at max_iter, 2 not converged at the library's sweep
    cap), ``pe_path`` and ``pe_kernel_ms`` (the whole call's)."""
    from . import device

    _single, ms = _one_topology(tabs)
    first = ms[0]
    n = np.shape(first["dst"])[0]
    policies = [_checked_policy(first, p) for p in policies]
    if not policies:
        raise ValueError("no policy to evaluate")
    if pairs is None:
        pairs = [(q, p) for q in range(len(policies)) for p in range(len(ms))]
    pairs = [(int(q), int(p)) for q, p in pairs]
    if not pairs:
        raise ValueError("no (policy, point) pair to evaluate")
    for q, p in pairs:
        if not 0 <= q < len(policies) or not 0 <= p < len(ms):
            raise ValueError(f"pair ({q}, {p}): no such policy or point")
    if states not in ("reachable", "all"):
        raise ValueError('states: expected "reachable" or "all"')
    if max_iter is not None and max_iter < 1:
        raise ValueError("max_iter: expected None or at least 1")
    if start is not None and _nesting(list(start)) == 3:
        if len(start) != len(ms):
            raise ValueError("start: expected one list per point")
        starts = [_checked_start(s, n) for s in start]
    else:
        starts = [_checked_start(start, n)] * len(ms)
    if len({len(s) for s in starts}) != 1:
        raise ValueError("start: every point needs the same number of start states")
    ctx = ctx or device.default_context()
    r = ctx.mdp_policy_evaluation(
        first["dst"], first["used"], first["valid"], first["rew"], first["prg"],
        np.stack([np.asarray(m["prb"], np.float64) for m in ms]),
        [p for _q, p in pairs], np.stack([policies[q] for q, _p in pairs]),
        theta=theta, discount=discount, max_iter=0 if max_iter is None else max_iter,
        states=states, start_state=[[s for s, _ in starts[p]] for _q, p in pairs],
        start_prob=[[pr for _, pr in starts[p]] for _q, p in pairs], path=path)
    return [dict(pe_reward=r["reward"][e], pe_progress=r["progress"][e],
                 pe_iter=int(r["iter"][e]), pe_delta=float(r["delta"][e]),
                 pe_status=int(r["status"][e]), pe_path=r["path_used"],
                 pe_kernel_ms=r["kernel_ms"]) for e in range(len(pairs))]


def _nesting(x):
    """Levels of lists / tuples above the scalars of ``x`` (an empty list counts as one)."""
    if not isinstance(x, (list, tuple)):
        return 0
    return 1 + max((_nesting(e) for e in x), default=0)


def _is_single(x):
    """Whether ``x`` is one MDP and not a list of them, by its shape alone: a packed dict is
    one MDP; a list or tuple that holds a packed dict is a list of MDPs; otherwise a tab
    nests four levels (states, actions, transitions, the four fields of a transition; lists
    or tuples alike) and a list of tabs five. Anything else is refused."""
    if isinstance(x, dict):
        return True
    if not isinstance(x, (list, tuple)):
        raise ValueError("expected a tab, a packed MDP or a list of them")
    if any(isinstance(e, dict) for e in x):
        return False
    depth = _nesting(x)
    if depth == 4:
        return True
    if depth == 5 or not x:
        return False
    raise ValueError("expected a tab (tab[s][i] = [(dst, p, reward, progress), ...]), a packed "
                     "MDP or a list of them; an MDP without any transition must be packed")


def _vi(tab, device, stop_delta):
    if device:
        return value_iteration_device(tab, stop_delta=stop_delta)
    return value_iteration(tab, stop_delta=stop_delta)


def solve(alpha, gamma, *, maximum_fork_length=20, horizon=100, stop_delta=1e-6, device=False):
    """The SSZ'16 Bitcoin MDP solved for PTO revenue; returns (model, states, vi).
    ``device``: solve on the device (the same result, plus ``vi_status``)."""
    model = BitcoinSM(alpha, gamma, maximum_fork_length)
    states, tab = compile_mdp(model)
    vi = _vi(ptmdp(tab, horizon), device, stop_delta)
    return model, states, vi


def solve_grid(alphas, gammas, *, maximum_fork_length=20, horizon=100, stop_delta=1e-6,
               ctx=None):
    """``solve`` for every (alpha, gamma), alpha-major, all points in one device call: a list
    of (model, states, vi), each what ``solve(alpha, gamma)`` returns."""
    models, all_states, tabs = [], [], []
    for alpha in alphas:
        for gamma in gammas:
            model = BitcoinSM(alpha, gamma, maximum_fork_length)
            states, tab = compile_mdp(model)
            models.append(model)
            all_states.append(states)
            tabs.append(pack(ptmdp(tab, horizon)))
    vis = value_iteration_device(tabs, stop_delta=stop_delta, ctx=ctx)
    return list(zip(models, all_states, vis))


def _policy_table_of(model, states, vi, dim):
    act = {}
    for sid, s in enumerate(states):
        acts = model.actions(s)
        if acts:
            act[s] = acts[int(vi["vi_policy"][sid])]
    table = np.zeros((dim, dim, 2), np.uint8)
    for h in range(dim):
        for a in range(dim):
            honest = OVERRIDE if a > h else (ADOPT if a < h else WAIT)
            for ev, fork, other in ((0, IRRELEVANT, RELEVANT), (1, RELEVANT, IRRELEVANT)):
                x = act.get((a, h, fork), act.get((a, h, other), honest))
                if x == MATCH and ev == 0 and (a, h, fork) not in act:
                    x = honest
                table[h, a, ev] = x
    return table.ravel()


def policy_table(alpha, gamma, *, dim=None, maximum_fork_length=20, horizon=100,
                 stop_delta=1e-6, device=False):
    """A `CPR_POLICY_TABLE` for `device.make_config(table=...)`: entry (h, a, event) =
    the MDP's action in state (a, h, IRRELEVANT) for event = ProofOfWork (0) and
    (a, h, RELEVANT) for event = Network (1) — the attacker's view after its own block or a
    defender's block; an active match (ACTIVE) is not observable by nakamoto_ssz and shares
    the ProofOfWork entry. States the MDP does not reach fall back to the other event's entry,
    else to honest play (nakamoto_ssz.ml:275-284). ``device``: solve on the device."""
    model, states, vi = solve(alpha, gamma, maximum_fork_length=maximum_fork_length,
                              horizon=horizon, stop_delta=stop_delta, device=device)
    return _policy_table_of(model, states, vi,
                            maximum_fork_length + 1 if dim is None else dim)


def policy_table_grid(alphas, gammas, *, dim=None, maximum_fork_length=20, horizon=100,
                      stop_delta=1e-6, ctx=None):
    """``policy_table`` for every (alpha, gamma), alpha-major, from one ``solve_grid``."""
    dim = maximum_fork_length + 1 if dim is None else dim
    return [_policy_table_of(model, states, vi, dim)
            for model, states, vi in solve_grid(alphas, gammas, horizon=horizon,
                                                maximum_fork_length=maximum_fork_length,
                                                stop_delta=stop_delta, ctx=ctx)]


# ---- the FC'16 abstract-model kernel (gym/rust/src/fc16.rs, cpr_amd/csrc/fc16_lane.h)

FC16_WAIT, FC16_ADOPT, FC16_OVERRIDE, FC16_MATCH = 0, 1, 2, 3  # fc16.rs:19-25 names
_FC16_NAME = {WAIT: FC16_WAIT, ADOPT: FC16_ADOPT, OVERRIDE: FC16_OVERRIDE, MATCH: FC16_MATCH}


def _fc16_table_of(model, states, vi, dim):
    act = {}
    for sid, s in enumerate(states):
        acts = model.actions(s)
        if acts:
            act[s] = _FC16_NAME[acts[int(vi["vi_policy"][sid])]]
    table = np.zeros((dim, dim, 3), np.uint8)
    for a in range(dim):
        for h in range(dim):
            honest = FC16_OVERRIDE if a > h else (FC16_ADOPT if h > a else FC16_WAIT)
            for fork in (IRRELEVANT, RELEVANT, ACTIVE):
                table[a, h, fork] = act.get((a, h, fork), honest)
    return table.ravel()


def fc16_table(alpha, gamma, *, dim=None, maximum_fork_length=20, horizon=100,
               stop_delta=1e-6, device=False):
    """A `CPR_FC16_POLICY_TABLE` (entry (a, h, fork) = an action name) from the solved
    SSZ'16 MDP: the MDP's action where it defines one, honest play elsewhere. ``device``:
    solve on the device."""
    model, states, vi = solve(alpha, gamma, maximum_fork_length=maximum_fork_length,
                              horizon=horizon, stop_delta=stop_delta, device=device)
    return _fc16_table_of(model, states, vi, maximum_fork_length + 1 if dim is None else dim)


def fc16_table_grid(alphas, gammas, *, dim=None, maximum_fork_length=20, horizon=100,
                    stop_delta=1e-6, ctx=None):
    """``fc16_table`` for every (alpha, gamma), alpha-major, from one ``solve_grid``."""
    dim = maximum_fork_length + 1 if dim is None else dim
    return [_fc16_table_of(model, states, vi, dim)
            for model, states, vi in solve_grid(alphas, gammas, horizon=horizon,
                                                maximum_fork_length=maximum_fork_length,
                                                stop_delta=stop_delta, ctx=ctx)]


def fc16_action_name(a, h, index):
    """The env's action rule (fc16.rs:49-60, 182): ``index`` selects from the offered list
    [Wait, Adopt, Override if a > h, Match if a >= h]; beyond the list it acts as Wait."""
    if index == 1:
        return FC16_ADOPT
    if index == 2:
        return FC16_OVERRIDE if a > h else (FC16_MATCH if a == h else FC16_WAIT)
    if index == 3:
        return FC16_MATCH if a > h else FC16_WAIT
    return FC16_WAIT


def fc16_table_from_net(net, dim, extra=None, ctx=None):
    """The `CPR_FC16_POLICY_TABLE` a deterministic ``device.PolicyNet`` plays in the FC16 env
    (`CPR_PROTO_FC16_ENV`): every (a, h, fork) with a, h < dim as an observation row through
    the device forward (argmax), the index mapped to an action name by the env's rule.
    ``extra`` replaces the network's constants (e.g. another alpha). The table is exact
    wherever a, h < dim: an episode of at most max_steps steps never leaves dim =
    max_steps + 2."""
    from . import _lib as L
    from . import device

    dim = int(dim)
    if not 1 <= dim <= 256:
        raise ValueError("dim: expected 1..256 (the table limit)")
    if extra is not None:
        if len(extra) != len(net.extra):
            raise ValueError(f"extra: expected {len(net.extra)} values")
        net = device.PolicyNet(net.pi, net.pi_head, net.vf, net.vf_head, extra=extra)
    x = np.arange(dim, dtype=np.float64)
    f = np.arange(3, dtype=np.float64)
    a, h, fork = (g.ravel() for g in np.meshgrid(x, x, f, indexing="ij"))
    obs = np.stack([a / (1.0 + a), h / (1.0 + h), fork / (1.0 + fork)], axis=1)
    cfg, keep = device.make_config(protocol=L.PROTO_FC16_ENV, alpha=0.25, gamma=0.5, n_lanes=1,
                                   policy=L.FC16_POLICY_HONEST)
    b = device.Batch(cfg, ctx=ctx, keep=keep)
    try:
        b.set_policy_net(net)
        index = b.policy_net_forward(obs, deterministic=True)[0]
    finally:
        b.close()
    table = np.zeros(obs.shape[0], np.uint8)
    for i, (ai, hi, ix) in enumerate(zip(a.astype(int), h.astype(int), index)):
        table[i] = fc16_action_name(ai, hi, int(ix))
    return table


def _fc16_threshold(p):
    t = p * 4294967296.0
    return 0 if t <= 0 else (4294967296 if t >= 4294967296.0 else int(t))


def fc16_policy_value(alpha, gamma, horizon, table, *, max_states=200_000):
    """Exact expected episode reward and progress of the device's FC16 lane under a table
    policy: the Markov chain of fc16.rs's transitions (a successful match adds reward h and
    progress 0, fc16.rs:109-110; the reward of the step that terminates is kept, fc16.rs:
    174-199) with the lane's draw probabilities (thresholds / 2^32), solved exactly over
    the states the policy reaches. Returns (E[reward], E[progress])."""
    pa = _fc16_threshold(alpha) / 4294967296.0
    pg = _fc16_threshold(gamma) / 4294967296.0
    pt = _fc16_threshold(1.0 / horizon) / 4294967296.0
    table = np.asarray(table, np.uint8).ravel()
    dim = int(round((table.size // 3) ** 0.5))

    def action(s):
        a, h, fork = s
        x = int(table[(min(a, dim - 1) * dim + min(h, dim - 1)) * 3 + fork])
        if (x == FC16_OVERRIDE and not a > h) or (x == FC16_MATCH and not a >= h):
            x = FC16_WAIT
        return x

    def transitions(s):
        a, h, fork = s
        x = action(s)
        if x == FC16_ADOPT:
            return [((1, 0, IRRELEVANT), pa, 0, h), ((0, 1, IRRELEVANT), 1 - pa, 0, h)]
        if x == FC16_OVERRIDE:
            return [((a - h, 0, IRRELEVANT), pa, h + 1, h + 1),
                    ((a - h - 1, 1, RELEVANT), 1 - pa, h + 1, h + 1)]
        if x == FC16_MATCH or fork == ACTIVE:
            return [((a + 1, h, ACTIVE), pa, 0, 0), ((a - h, 1, RELEVANT), (1 - pa) * pg, h, 0),
                    ((a, h + 1, RELEVANT), (1 - pa) * (1 - pg), 0, 0)]
        return [((a + 1, h, IRRELEVANT), pa, 0, 0), ((a, h + 1, RELEVANT), 1 - pa, 0, 0)]

    starts = [(1, 0, IRRELEVANT), (0, 1, IRRELEVANT)]
    ids, order, queue = {}, [], deque(starts)
    for s in starts:
        ids[s] = len(order)
        order.append(s)
    tr = []
    while queue:
        s = queue.popleft()
        row = transitions(s)
        tr.append(row)
        for d, _p, _r, _g in row:
            if d not in ids:
                if len(order) >= max_states:
                    raise ValueError("the policy reaches more than max_states states")
                ids[d] = len(order)
                order.append(d)
                queue.append(d)
    n = len(order)
    m = np.eye(n)
    rhs_r = np.zeros(n)
    rhs_g = np.zeros(n)
    for s_id, row in enumerate(tr):
        for d, p, r, g in row:
            cont = (1.0 - pt) ** g  # no termination draw fires over g units of progress
            m[s_id, ids[d]] -= p * cont
            rhs_r[s_id] += p * r
            rhs_g[s_id] += p * g
    v_r = np.linalg.solve(m, rhs_r)
    v_g = np.linalg.solve(m, rhs_g)
    return (pa * v_r[0] + (1 - pa) * v_r[1], pa * v_g[0] + (1 - pa) * v_g[1])


# ---- table policies as MDP policies, and the revenue of Q policies at P points

def fc16_honest_table(dim):
    """Honest play as a `CPR_FC16_POLICY_TABLE` (fc16_lane.h ``POLICY_HONEST``)."""
    table = np.zeros((dim, dim, 3), np.uint8)
    for a in range(dim):
        for h in range(dim):
            table[a, h, :] = FC16_OVERRIDE if a > h else (FC16_ADOPT if h > a else FC16_WAIT)
    return table.ravel()


def fc16_sm1_table(dim):
    """SM1 (sapirshtein-2016-sm1) as a `CPR_FC16_POLICY_TABLE` (fc16_lane.h ``POLICY_SM1``)."""
    table = np.zeros((dim, dim, 3), np.uint8)
    for a in range(dim):
        for h in range(dim):
            if h > a:
                x = FC16_ADOPT
            elif h == 1 and a == 1:
                x = FC16_MATCH
            elif h == a - 1 and h >= 1:
                x = FC16_OVERRIDE
            else:
                x = FC16_WAIT
            table[a, h, :] = x
    return table.ravel()


_FC16_MODEL = {name: act for act, name in _FC16_NAME.items()}


def mdp_policy_from_table(model, states, table, kind):
    """The MDP policy that a table plays: per state of ``states`` (``compile_mdp``'s order)
    the index of the table's action in ``model.actions(state)``, and a final -1 for the
    terminal state that ``ptmdp`` appends.

    ``kind="nakamoto"``: a `CPR_POLICY_TABLE` over (h, a, event), event = Network (1) for
    fork RELEVANT and ProofOfWork (0) for IRRELEVANT and ACTIVE, as ``policy_table`` writes
    it. ``kind="fc16"``: a `CPR_FC16_POLICY_TABLE` over (a, h, fork) with the env's legality
    rule (``fc16_policy_value``: Override without a > h and Match without a >= h act as
    Wait). a and h beyond the table read its last row or column. An action the model does
    not offer in a state (Wait at a truncated state, Match without a relevant fork, ...)
    becomes Override if a > h, else Adopt."""
    table = np.asarray(table, np.uint8).ravel()
    if kind == "nakamoto":
        dim = int(round((table.size // 2) ** 0.5))
        if dim < 1 or dim * dim * 2 != table.size:
            raise ValueError("table: expected dim * dim * 2 entries")
    elif kind == "fc16":
        dim = int(round((table.size // 3) ** 0.5))
        if dim < 1 or dim * dim * 3 != table.size:
            raise ValueError("table: expected dim * dim * 3 entries")
    else:
        raise ValueError('kind: expected "nakamoto" or "fc16"')
    if table.max() > 3:
        raise ValueError("table: an entry is no action")
    policy = np.full(len(states) + 1, -1, np.int64)
    for sid, (a, h, fork) in enumerate(states):
        acts = model.actions((a, h, fork))
        ca, ch = min(a, dim - 1), min(h, dim - 1)
        if kind == "nakamoto":
            x = int(table[(ch * dim + ca) * 2 + (1 if fork == RELEVANT else 0)])
        else:
            x = int(table[(ca * dim + ch) * 3 + fork])
            if (x == FC16_OVERRIDE and not a > h) or (x == FC16_MATCH and not a >= h):
                x = FC16_WAIT
            x = _FC16_MODEL[x]
        if x not in acts:
            x = OVERRIDE if a > h else ADOPT
        policy[sid] = acts.index(x)
    return policy


def revenue_matrix(alphas, gammas, policies=None, *, maximum_fork_length=20, horizon=100,
                   stop_delta=1e-6, theta=1e-6, ctx=None):
    """The PTO revenue of Q policies at P = len(alphas) * len(gammas) points (alpha-major), all
    evaluations in one ``policy_evaluation_device`` call after one ``solve_grid``: every
    point's optimum, honest play, SM1 and the tables of ``policies`` (a dict label -> (table,
    kind) or a list of (table, kind), ``kind`` as for ``mdp_policy_from_table``), each
    evaluated at every point over the states it reaches from the model's start states.
    revenue = sum start * pe_reward / sum start * pe_progress over the start states.

    Returns a dict: ``revenue`` [Q][P]; ``policies`` (Q labels: "optimum(alpha,gamma)" per
    point, "honest", "sm1", then the given ones) and ``points`` (P (alpha, gamma) pairs);
    ``vi_revenue`` [P], the same ratio of the optimum's own value-iteration vectors;
    ``pe_iter`` and ``pe_status`` [Q][P]."""
    solved = solve_grid(alphas, gammas, maximum_fork_length=maximum_fork_length,
                        horizon=horizon, stop_delta=stop_delta, ctx=ctx)
    points = [(m.alpha, m.gamma) for m, _s, _v in solved]
    model, states, _vi = solved[0]  # the topology does not depend on the point
    tabs = [pack(ptmdp(compile_mdp(m)[1], horizon)) for m, _s, _v in solved]
    starts = [[(0, m.start()[0][1]), (1, m.start()[1][1])] for m, _s, _v in solved]
    labels = [f"optimum({a:g},{g:g})" for a, g in points] + ["honest", "sm1"]
    pols = [np.asarray(vi["vi_policy"], np.int64) for _m, _s, vi in solved]
    dim = maximum_fork_length + 1
    given = list(policies.items()) if isinstance(policies, dict) else \
        [(f"table{i}", tk) for i, tk in enumerate(policies or [])]
    for table in (fc16_honest_table(dim), fc16_sm1_table(dim)):
        pols.append(mdp_policy_from_table(model, states, table, "fc16"))
    for label, (table, kind) in given:
        pols.append(mdp_policy_from_table(model, states, table, kind))
        labels.append(label)
    pes = policy_evaluation_device(tabs, pols, theta=theta, start=starts, ctx=ctx)
    n_p = len(points)

    def ratio(reward, progress, start):
        num = sum(p * reward[s] for s, p in start)
        den = sum(p * progress[s] for s, p in start)
        return num / den if den else 0.0

    revenue = np.zeros((len(pols), n_p))
    iters = np.zeros((len(pols), n_p), np.int64)
    status = np.zeros((len(pols), n_p), np.int32)
    for e, pe in enumerate(pes):
        q, p = divmod(e, n_p)
        revenue[q, p] = ratio(pe["pe_reward"], pe["pe_progress"], starts[p])
        iters[q, p], status[q, p] = pe["pe_iter"], pe["pe_status"]
    vi_revenue = np.array([ratio(vi["vi_value"], vi["vi_progress"], starts[p])
                           for p, (_m, _s, vi) in enumerate(solved)])
    return dict(revenue=revenue, policies=labels, points=points, vi_revenue=vi_revenue,
                pe_iter=iters, pe_status=status)
