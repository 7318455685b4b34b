"""TEST INFRASTRUCTURE ONLY: the FC'16 abstract model as an environment, pure Python.

Restates gym/rust/src/fc16.rs FC16SSZwPT (reset, step by action index) on the keyed stream
of cpr_amd/csrc/fc16_lane.h (oracle_py.keyed_block), independent of the library:

  start          block(0, TAG | 1).w0 < t_alpha -> (a, h) = (1, 0) else (0, 1)
  step j         block(j, TAG): w0 < t_alpha mining, w1 < t_gamma network
  termination i  word i & 3 of block(j, TAG | 0x100000 | i >> 2) < t_term, one per unit of
                 progress of the step

Actions index the offered list [Wait, Adopt, Override if a > h, Match if a >= h]; an index
beyond the list acts as entry 0 (fc16.rs:49-60, 182). Observation x / (1 + x) of (a, h,
fork) in float64 (fc16.rs:61-73). max_steps truncates (status CPR_ST_CAPACITY = 32), which
the reference env leaves to gymnasium's TimeLimit.
"""

import oracle_py as O

WAIT, ADOPT, OVERRIDE, MATCH = 0, 1, 2, 3
NAMES = ("Wait", "Adopt", "Override", "Match")
IRRELEVANT, RELEVANT, ACTIVE = 0, 1, 2
TAG = 0x40000000
ST_CAPACITY = 32


def threshold(p):
    t = p * 4294967296.0
    return 0 if t <= 0 else (4294967296 if t >= 4294967296.0 else int(t))


def offered(a, h):
    acts = [WAIT, ADOPT]
    if a > h:
        acts.append(OVERRIDE)
    if a >= h:
        acts.append(MATCH)
    return acts


def action_name(a, h, index):
    acts = offered(a, h)
    return acts[index] if 0 <= index < len(acts) else acts[0]


def index_of(a, h, name):
    """The index that plays `name` in state (a, h); a name not offered plays Wait, as the
    fused lane does (fc16_lane.h)."""
    acts = offered(a, h)
    return acts.index(name) if name in acts else 0


def observe(a, h, fork):
    return [float(x) / (1.0 + float(x)) for x in (a, h, fork)]


class Fc16EnvRef:
    def __init__(self, seed, alpha, gamma, horizon, max_steps=None):
        self.seed = seed
        self.ta, self.tg, self.tt = threshold(alpha), threshold(gamma), threshold(1.0 / horizon)
        self.max_steps = max_steps if max_steps else 1 << 30
        self.ep = None

    def set_alpha(self, alpha):
        self.ta = threshold(alpha)

    def reset(self, ep):
        self.ep = int(ep)
        if int(O.keyed_block(self.seed, self.ep, 0, TAG | 1)[0]) < self.ta:
            self.a, self.h = 1, 0
        else:
            self.a, self.h = 0, 1
        self.fork = IRRELEVANT
        self.reward = self.progress = self.steps = 0
        self.status = 0
        self.last_name = None
        return observe(self.a, self.h, self.fork)

    def step(self, index):
        """(obs, reward, terminated, truncated); last_name = the action that was applied."""
        a, h, fork = self.a, self.h, self.fork
        name = action_name(a, h, int(index))
        self.last_name = name
        j = self.steps
        w = O.keyed_block(self.seed, self.ep, j, TAG)
        mining = int(w[0]) < self.ta
        r = g = 0
        if name == ADOPT:
            a, h, fork, g = (1, 0, IRRELEVANT, h) if mining else (0, 1, IRRELEVANT, h)
        elif name == OVERRIDE:
            r = g = h + 1
            a, h, fork = (a - h, 0, IRRELEVANT) if mining else (a - h - 1, 1, RELEVANT)
        elif name == MATCH or fork == ACTIVE:
            if mining:
                a, fork = a + 1, ACTIVE
            elif int(w[1]) < self.tg:
                r = h
                a, h, fork = a - h, 1, RELEVANT
            else:
                h, fork = h + 1, RELEVANT
        elif mining:
            a, fork = a + 1, IRRELEVANT
        else:
            h, fork = h + 1, RELEVANT
        self.a, self.h, self.fork = a, h, fork
        self.reward += r
        self.progress += g
        self.steps += 1
        term = False
        for i in range(g):
            if i % 4 == 0:
                t = O.keyed_block(self.seed, self.ep, j, TAG | 0x100000 | (i >> 2))
            if int(t[i % 4]) < self.tt:
                term = True
                break
        trunc = not term and self.steps >= self.max_steps
        if trunc:
            self.status |= ST_CAPACITY
        return observe(a, h, fork), float(r), term, trunc

    def info(self):
        """The step infos of the device lane (the fused record's mapping)."""
        return dict(episode_reward_attacker=float(self.reward),
                    episode_reward_defender=float(self.progress - self.reward),
                    episode_progress=float(self.progress), episode_chain_time=0.0,
                    episode_sim_time=0.0, episode_n_steps=self.steps,
                    episode_n_activations=self.steps + 1, head_height=self.progress,
                    head_miner=-1, status=self.status)
