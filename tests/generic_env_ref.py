"""TEST INFRASTRUCTURE ONLY: the generic release/consider env over Nakamoto, pure Python.

Restates gym/rust/src/generic/mod.rs Env with proto/nakamoto.rs (the reference's Nakamoto-v0)
as a literal graph: a list of parent lists, view enums per block, full rescans for the action
lists, entry points found by search, histories as Python lists. It shares nothing with the
incremental structures of cpr_amd/csrc/generic_lane.h. Draws come from the keyed stream
(oracle_py.keyed_block), laid out as the lane documents:

  Continue at step j   block(j, TAG): w1 < t_gamma fast in communicate, w0 < t_alpha attacker
                       mines
  shutdown at step j   w2 < t_gamma of the same block
  termination unit i   word i & 3 of block(j, TAG | 0x100000 | i >> 2) < t_term, one per unit
                       of the step's progress before shutdown

Actions are the reference's integers (mod.rs:214-220): 0 Continue, -(i+1) Release(i), +(i+1)
Consider(i), clamped to +-256. The observation and the action codec are numpy float32.
max_steps truncates (status CPR_ST_CAPACITY = 32, no shutdown); an episode that is over
ignores further steps.

Independent anchors (computed from the keyed words alone, no DAG):

honest_counter: generic_honest_action plays Release(0) while something can be released, else
Consider(0) while something can be considered, else Continue. A Continue mines one block; it
is either the attacker's (withheld, the only releasable block) or a defender's (the only
ignored block), so the next step releases or considers it, and the step after is the next
Continue, whose communicate delivers it: it is one higher than the defenders' entry, so they
adopt it (nakamoto.rs:27-33). Hence steps 0, 2, 4, ... are Continue, Continue 2k (k >= 1)
has progress 1, pays the miner of block k - 1 (w0 of block(2k - 2, TAG) < t_alpha: attacker)
and draws one termination word, word 0 of block(2k, TAG | 0x100000). When it fires, shutdown
delivers the block mined at step 2k as well (released if withheld), again one higher. So
every mined block ends on the defenders' chain, progress is the number of blocks, the
attacker's reward is the number of attacker miner draws, and nothing is ever rewritten.

continue_counter: with Continue alone the attacker never releases and never considers a
defender block, so its blocks form one private chain on genesis of length a (mine_attacker
mines on the attacker's entry, which moves to each own block, mod.rs:719-721), and every
defender block extends the defenders' chain and is delivered by the next Continue (progress 1,
defender reward 1, one termination word at that step). At termination in step j, d defender
blocks are delivered and the block mined at step j is on the wire if it is a defender's.
shutdown (mod.rs:728-758) releases the a attacker blocks in order and delivers them before
the wire block if w2 < t_gamma, after it otherwise. A delivered block becomes the defenders'
entry iff it is strictly higher (nakamoto.rs:27-33), the attacker blocks have heights 1 .. a,
so the defenders end on the attacker chain iff a > d + (1 if the wire block came first). If
they do, the second track_defender_chain compares the a attacker blocks with the tracked
history of d defender blocks: progress a - d, attacker reward a, defender reward -d, d blocks
rewritten; a wire block delivered first is not in the tracked history and one delivered after
is not higher than a. If they do not, a wire block is adopted: progress 1, defender 1.
"""

import numpy as np

import oracle_py as O

TAG = 0xB0000000
ST_CAPACITY, ST_REFERENCE_RAISES = 32, 64
IGNORED, CONSIDERED, AENTRY = 0, 1, 2
UNKNOWN, KNOWN, DENTRY = 0, 1, 2
HONEST, WITHHELD, RELEASED = 0, 1, 2
F = np.float32


class ReferenceRaises(Exception):
    pass


def _check(cond, what):
    if not cond:
        raise ReferenceRaises(what)


def threshold(p):
    t = p * 4294967296.0
    return 0 if t <= 0 else (4294967296 if t >= 4294967296.0 else int(t))


def clamp_action(a):
    return max(-256, min(256, int(a)))


def encode_action(a):
    """mod.rs:236-248 on the integer form, float32."""
    if a == 0:
        return F(0.0)
    x = F(clamp_action(a))
    return F(x / F(F(1.0) + abs(x)))


def _round_half_away(x):
    r = np.trunc(x)
    if abs(F(x - r)) >= F(0.5):
        r = F(r + np.copysign(F(1.0), x))
    return F(r)


def decode_action(a):
    """mod.rs:250-279: float32 action to the integer form; raises outside [-1, 1]."""
    a = F(a)
    if not (a >= F(-1.0)) or not (a <= F(1.0)):
        raise ValueError(f"invalid action: {a} outside [-1, 1]")
    if a == F(-1.0):
        return -256
    if a == F(1.0):
        return 256
    with np.errstate(divide="ignore", over="ignore"):
        x = F(-a) / F(a - F(1.0)) if a >= 0 else a / F(a + F(1.0))
    x = _round_half_away(F(x))
    if x < -256:
        return -256
    if x < 0:
        return -(int(-x - 1) + 1)
    if x > 256:
        return 256
    if x > 0:
        return int(x - 1) + 1
    return 0


def head_action(index, k):
    """The categorical head of 1 + 2K actions to the integer form."""
    if index <= 0 or index > 2 * k:
        return 0
    return -index if index <= k else index - k


def honest_action(n_release, n_consider):
    return -1 if n_release > 0 else (1 if n_consider > 0 else 0)


class GenericNakamotoRef:
    def __init__(self, seed, alpha, gamma, horizon, max_steps):
        self.seed = seed
        self.ta, self.tg = threshold(alpha), threshold(gamma)
        self.tt = threshold(1.0 / horizon)
        self.max_steps = int(max_steps)
        self.ep = None
        self.events = set()  # what the fuzz reached (test_generic_env_host.py)

    def set_alpha(self, alpha):
        self.ta = threshold(alpha)

    # ------------------------------------------------------------ graph (mod.rs:65-87)
    def _parents(self, b):
        return self.par[b]

    def _children(self, b):
        return [x for x in range(len(self.par)) if b in self.par[x]]

    def _add(self, parents, height, av, dv, nv):
        self.par.append(list(parents))
        self.height.append(height)
        self.av.append(av)
        self.dv.append(dv)
        self.nv.append(nv)
        return len(self.par) - 1

    def _entry(self, defender):  # mod.rs:633-645
        if defender:
            return self.dv.index(DENTRY)
        return self.av.index(AENTRY)

    # ------------------------------------------------------------ proto/nakamoto.rs
    def _mining(self, ep):  # :19-25
        return [ep], self.height[ep] + 1

    def _update(self, ep, b):  # :27-33
        return b if self.height[b] > self.height[ep] else ep

    def _pred(self, b):  # :39-46
        p = self._parents(b)
        return p[0] if p else None

    def _history(self, b):  # mod.rs:854-862
        v = []
        while b is not None:
            v.insert(0, b)
            b = self._pred(b)
        return v

    # ------------------------------------------------------------ mod.rs:286-314
    def _available(self):
        rel, con = [], []
        for b in range(len(self.par)):
            if self.nv[b] == WITHHELD and all(self.nv[p] != WITHHELD for p in self._parents(b)):
                rel.append(b)
            if self.av[b] == IGNORED and all(self.av[p] != IGNORED for p in self._parents(b)):
                con.append(b)
        return rel, con

    def reset(self, ep):
        self.ep = int(ep)
        self.par, self.height, self.av, self.dv, self.nv = [], [], [], [], []
        self._add([], 0, AENTRY, DENTRY, HONEST)
        self.rel, self.con = self._available()
        self.ca = 0
        self.hist = [0]
        self.era = self.erd = self.eprog = self.rewrites = 0
        self.mined = self.steps = 0
        self.status = 0
        self.over = False
        self.last = dict(progress=0, reward_attacker=0, reward_defender=0, rewrite=0, time=0)
        return self.observe()

    # ------------------------------------------------------------ mod.rs:647-693
    def _deliver(self, b):
        _check(self.dv[b] == UNKNOWN, "repeated delivery")
        _check(all(self.dv[p] != UNKNOWN for p in self._parents(b)), "missing dependencies")
        self.dv[b] = KNOWN
        ep = self._entry(True)
        self.dv[ep] = KNOWN
        self.dv[self._update(ep, b)] = DENTRY

    def _consider(self, b):
        _check(self.av[b] == IGNORED, "repeated consider")
        _check(all(self.av[p] != IGNORED for p in self._parents(b)), "missing dependencies")
        self.av[b] = CONSIDERED
        ep = self._entry(False)
        self.av[ep] = CONSIDERED
        self.av[self._update(ep, b)] = AENTRY  # on the defender view (mod.rs:678): heights only

    def _release(self, b):
        _check(self.nv[b] == WITHHELD, "unsuitable block")
        _check(all(self.nv[p] != WITHHELD for p in self._parents(b)), "missing dependencies")
        self.nv[b] = RELEASED

    # ------------------------------------------------------------ mod.rs:715-819
    def _communicate(self, fast):
        n = range(len(self.par))
        from_attacker = [x for x in n if self.dv[x] == UNKNOWN and self.nv[x] == RELEASED]
        from_defender = [x for x in n if self.dv[x] == UNKNOWN and self.nv[x] == HONEST]
        _check(len(from_defender) <= 1, "abnormal honest mining")
        for b in (from_attacker + from_defender) if fast else (from_defender + from_attacker):
            self._deliver(b)

    def _continue(self, w):
        self._communicate(int(w[1]) < self.tg)
        if int(w[0]) < self.ta:
            parents, h = self._mining(self._entry(False))
            b = self._add(parents, h, IGNORED, UNKNOWN, WITHHELD)
            self._consider(b)
        else:
            parents, h = self._mining(self._entry(True))
            self._add(parents, h, IGNORED, UNKNOWN, HONEST)
        self.mined += 1

    def _shutdown(self, fast):
        from_attacker, from_defender = [], []
        for b in range(len(self.par)):
            nv, dv = self.nv[b], self.dv[b]
            if nv == WITHHELD:
                self._release(b)
                from_attacker.append(b)
            if nv == HONEST and dv == UNKNOWN:
                from_defender.append(b)
        _check(len(from_defender) <= 1, "env logic broken?")
        self.events.add(("shutdown", fast, len(from_defender) == 1))
        for b in (from_attacker + from_defender) if fast else (from_defender + from_attacker):
            self._deliver(b)

    # ------------------------------------------------------------ mod.rs:557-623
    def _track(self):
        cur = self._history(self._entry(True))
        old = self.hist
        _check(cur[0] == old[0], "genesis must not change")
        _check(len(cur) >= len(old), "shrinking history")
        i = 0
        while i < len(old) and cur[i] == old[i]:
            i += 1
        first = i
        prg = ra = rd = upd = 0
        for b in cur[first:]:
            prg += 1
            if self.nv[b] == HONEST:
                rd += 1
            else:
                ra += 1
        for b in old[first:]:
            upd += 1
            prg -= 1
            if self.nv[b] == HONEST:
                rd -= 1
            else:
                ra -= 1
        self.hist = cur
        return upd, prg, ra, rd

    def _common_ancestor(self):  # mod.rs:864-882
        a = self._history(self._entry(False))
        d = self._history(self._entry(True))
        common = []
        for x, y in zip(a, d):
            if x != y:
                break
            common.append(x)
        return common[-1]

    # ------------------------------------------------------------ mod.rs:446-555
    def step(self, action):
        """(obs, attacker reward of the step, terminated, truncated)."""
        if self.over:
            self.last = dict(progress=0, reward_attacker=0, reward_defender=0, rewrite=0, time=0)
            return self.observe(), 0.0, False, False
        j = self.steps
        action = clamp_action(action)
        # guarded_action
        if action < 0:
            n, i = len(self.rel), -action - 1
        elif action > 0:
            n, i = len(self.con), action - 1
        if action != 0:
            if n < 1:
                self.events.add(("empty", action < 0))
                action = 0
            elif i >= n:
                self.events.add(("clamped", action < 0))
                i = n - 1
        time = 0
        w = None
        if action < 0:
            self._release(self.rel[i])
        elif action > 0:
            self._consider(self.con[i])
        else:
            w = O.keyed_block(self.seed, self.ep, j, TAG)
            self._continue(w)
            time = 1
        self.rel, self.con = self._available()
        if len(self.rel) >= 2:
            self.events.add("release>=2")
        if len(self.con) >= 2:
            self.events.add("consider>=2")
        self.ca = self._common_ancestor()
        upd, prg, ra, rd = self._track()
        _check(prg >= 0, "negative progress")
        term = False
        for u in range(prg):
            if u % 4 == 0:
                t = O.keyed_block(self.seed, self.ep, j, TAG | 0x100000 | (u >> 2))
            if int(t[u % 4]) < self.tt:
                term = True
                break
        if term:
            self._shutdown(int(w[2]) < self.tg)
            upd2, prg2, ra2, rd2 = self._track()
            upd, prg, ra, rd = upd + upd2, prg + prg2, ra + ra2, rd + rd2
        self.steps += 1
        self.era += ra
        self.erd += rd
        self.eprog += prg
        self.rewrites += upd
        self.last = dict(progress=prg, reward_attacker=ra, reward_defender=rd, rewrite=upd,
                         time=time)
        if upd > 0:
            self.events.add("rewrite")
        if ra < 0:
            self.events.add("negative")
        trunc = not term and self.steps >= self.max_steps
        if trunc:
            self.status |= ST_CAPACITY
            self.events.add("truncated")
        self.over = term or trunc
        return self.observe(), float(ra), term, trunc

    # ------------------------------------------------------------ mod.rs:884-911, nakamoto.rs:71-104
    def _base(self):
        atk, dfn = self._entry(False), self._entry(True)
        ch, ah, dh, mf = self.height[self.ca], self.height[atk], self.height[dfn], 0
        children = [b for b in self._children(dfn) if self.nv[b] == HONEST]
        if children:
            _check(len(children) == 1, "bug in protocol spec or env?")
            c = children[0]
            _check(len(self._children(c)) == 0, "bug in proto spec or env?")
            _check(self.dv[c] == UNKNOWN, "bug in proto spec or env?")
            _check(self.height[c] == dh + 1, "bug in proto spec or env?")
            dh += 1
            mf = 1
        return ah - ch, dh - ch, mf

    def observe(self):
        a, d, mf = self._base()
        o = [F(a), F(d), F(mf)]
        n = len(self.rel)
        o.append(encode_action(-(((n - 1) & 255) + 1)) if n > 0 else F(0))
        n = len(self.con)
        o.append(encode_action(((n - 1) & 255) + 1) if n > 0 else F(0))
        return np.array(o, dtype=np.float32)

    def fields(self):
        """cpr_observe_fields: a, d, match feasible, n_release, n_consider, n_blocks, the last
        step's rewrite count."""
        a, d, mf = self._base()
        return [a, d, mf, len(self.rel), len(self.con), len(self.par), self.last["rewrite"]]

    def info(self):
        """The step infos of the device lane (StepBuffers)."""
        return dict(episode_reward_attacker=float(self.era),
                    episode_reward_defender=float(self.erd),
                    episode_progress=float(self.eprog), episode_chain_time=0.0,
                    episode_sim_time=0.0, episode_n_steps=self.steps,
                    episode_n_activations=self.mined + 1,
                    head_height=self.height[self._entry(True)], head_miner=-1,
                    status=self.status)


# ---------------------------------------------------------------- the counter models

def _word(seed, ep, j, tag, k):
    return int(O.keyed_block(seed, ep, j, tag)[k])


def honest_counter(seed, ep, alpha, gamma, horizon, max_steps):
    """generic_honest_action's episode from the draws alone (module docstring): dict of
    reward_attacker, reward_defender, progress, steps, rewrite (last step), terminated,
    truncated."""
    ta, tt = threshold(alpha), threshold(1.0 / horizon)
    ra = rd = steps = 0
    term = False
    miners = []  # attacker? per block
    for j in range(max_steps):
        steps = j + 1
        if j % 2:
            continue  # release or consider the block of the Continue before
        k = j // 2
        if k >= 1:
            ra, rd = ra + miners[k - 1], rd + (not miners[k - 1])
            term = _word(seed, ep, j, TAG | 0x100000, 0) < tt
        miners.append(_word(seed, ep, j, TAG, 0) < ta)
        if term:
            ra, rd = ra + miners[k], rd + (not miners[k])
            break
    return dict(reward_attacker=ra, reward_defender=rd, progress=ra + rd, steps=steps,
                rewrite=0, terminated=term, truncated=not term)


def continue_counter(seed, ep, alpha, gamma, horizon, max_steps):
    """The always-Continue episode from the draws alone (module docstring)."""
    ta, tg, tt = threshold(alpha), threshold(gamma), threshold(1.0 / horizon)
    a = d = steps = 0
    wire = term = False
    for j in range(max_steps):
        steps = j + 1
        if wire:  # the defender block of step j - 1 arrives
            d += 1
            term = _word(seed, ep, j, TAG | 0x100000, 0) < tt
        w = O.keyed_block(seed, ep, j, TAG)
        wire = not int(w[0]) < ta
        a += not wire
        if term:
            slow_first = wire and not int(w[2]) < tg
            if a > d + slow_first:
                # the d delivered defender blocks paid d before and are all dropped now
                return dict(reward_attacker=a, reward_defender=0, progress=a, steps=steps,
                            rewrite=d, terminated=True, truncated=False)
            d += wire
            break
    return dict(reward_attacker=0, reward_defender=d, progress=d, steps=steps, rewrite=0,
                terminated=term, truncated=not term)
