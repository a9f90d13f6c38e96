"""The episode-statistics update rule and outcome codes (libzombsole_amd/csrc/zs_episode.hpp) restated in Python over
the oracle's step results and canonical states (OracleEnv.step / .state()).  Nothing here comes from the engine.

Per env: run_ret [R] and closed (running), last_ret [R] and last [8] (the last finished episode), tot [8] (uint32
counters, sums mod 2**32) and sum_ret [R].  R = 1 on the single surface, A on the multi surface.  Floats are Python
floats (IEEE doubles): one add per step, in step order."""
import numpy as np

from libzombsole_amd import _abi

LIFE = 2  # a canonical state's agents / players rows: [x, y, life, weapon]
M32 = 0xffffffff


def outcome_code(rules, state, done, trunc):
    """last[1] of a terminal step that left `state`: 1 won, 2 lost, 3 truncated with no agent alive, 4 truncated with
    one alive (the TimeLimit); | 256 when done and truncated are both set."""
    team = state["agents"] + state["players"]
    alive = sum(1 for p in team if p[LIFE] > 0)
    won = 2 * alive >= len(team) if rules == _abi.RULES_EVACUATION else alive > 0
    agent_alive = any(p[LIFE] > 0 for p in state["agents"])
    code = (1 if won else 2) if done else (4 if agent_alive else 3)
    return code | (256 if done and trunc else 0)


class EnvModel(object):
    def __init__(self, R, rules):
        self.R, self.rules = R, rules
        self.run, self.closed = [0.0] * R, 0
        self.last_ret, self.last = [0.0] * R, [0] * 8
        self.tot, self.sum_ret = [0] * 8, [0.0] * R
        self.length = 0  # steps since the reset (the TimeLimit's count)

    def reset(self):
        """Rule 1: the env's reset (explicit, or the autoreset step)."""
        self.run, self.closed, self.length = [0.0] * self.R, 0, 0

    def clear(self):
        """zs_episode_stats_clear: the last episode and the totals; the running part stays."""
        self.last_ret, self.last = [0.0] * self.R, [0] * 8
        self.tot, self.sum_ret = [0] * 8, [0.0] * self.R

    def step(self, rew, done, trunc, state, triple):
        """Rules 2 to 4 for a step that ticked: the oracle's rewards (its first R), flags and the state the step
        left; triple: the (initial_zombies, minimum_zombies, max_episode_steps) the episode runs under."""
        self.length += 1
        if self.closed:
            return
        for r in range(self.R):
            self.run[r] = self.run[r] + float(rew[r])
        if not (done or trunc):
            return
        code = outcome_code(self.rules, state, done, trunc)
        _, deaths, zd = state["ctr"]
        self.last_ret = list(self.run)
        t = self.tot
        t[0] = (t[0] + 1) & M32
        t[code & 255] = (t[code & 255] + 1) & M32
        t[5], t[6], t[7] = (t[5] + self.length) & M32, (t[6] + zd) & M32, (t[7] + deaths) & M32
        self.last = [self.length, code, zd, deaths, triple[0], triple[1], triple[2], t[0]]
        for r in range(self.R):
            self.sum_ret[r] = self.sum_ret[r] + self.run[r]
        self.closed = 1

    def copy_running_from(self, other):
        """zs_restore / clone: only the running part belongs to an env."""
        self.run, self.closed, self.length = list(other.run), other.closed, other.length


def hexes(values):
    """Floats as hex strings (bit-exact comparison, readable on a mismatch)."""
    return [float(v).hex() for v in np.asarray(values, dtype=np.float64).ravel()]


def snapshot(models):
    """The five tensors of zs_episode_stats_get for a list of env models, floats as hex strings, plus "closed"."""
    return {"run_ret": [hexes(m.run) for m in models], "last_ret": [hexes(m.last_ret) for m in models],
            "sum_ret": [hexes(m.sum_ret) for m in models], "last": [list(m.last) for m in models],
            "tot": [list(m.tot) for m in models], "closed": [m.closed for m in models]}
