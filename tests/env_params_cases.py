"""Per-env zombie counts and time limits (ZS_FLAG_ENV_PARAMS): the table of cases of test_env_params_plan.py (CPU: the
oracle alone shows what every row claims) and test_env_params.py (GPU: every env at every step against an oracle env
of its own config), and the runner the GPU cases share.

A handle's config gives the caps (I initial, M minimum zombies); env e of a row runs the triple
TRIPLES(I, M)[e % 13].  The list holds initial 0, 1 and I, minimum 0 and M, max_episode_steps 0, 1 and values the
episodes reach (3 to 6), and is ordered so that the 13 envs of a G = 64 row take every triple once.  What a row
must show in three envs or more, by the oracle alone (census()):
  timelimit   a TimeLimit truncation at the env's own limit (the episode's length equals max_steps_e, not done);
  respawn     a respawn in an env with 0 < minimum_e < M;
  below       an env with minimum_e = 0 and initial_e >= 1 whose zombies number less than M at some step and never
              more again until the episode, or the run, ends (nothing respawns there);
  win         an extermination win (done, the agents rewarded +10) in an env with initial_e < I.
Rules are extermination throughout.  Zombies go into the lowest free zombie slots, so env e's state is, slot for slot,
the state of an oracle env built with (initial_e, minimum_e, max_steps_e); the slots past A + P + max(initial_e,
minimum_e) stay absent.

Rows: G = 1, 8, 16 and 64; k_step (the reset fused into the step launch) and k_tick with k_reset on its side stream;
respawn by the tick's leader (defer_respawn = -1) and by k_respawn (+1); eager steps and step_graph; both surfaces;
the crowded 12 x 6 map of test_conflict_census.py and bridge64.  Env counts are step_instantiations.ENVS (odd, a
partial last workgroup), 24 steps.
"""
import numpy as np

import step_instantiations as S
from libzombsole_amd import _abi
from libzombsole_amd import actions as A
from libzombsole_amd.maps import Map

from test_conflict_census import MELEE_MAP

STEPS = S.STEPS
CHANGE_AFTER = 8  # case 2: the step after which half the envs get another triple


def TRIPLES(I, M):
    assert I >= 3 and M >= 3
    return [(0, 0, 4), (1, 0, 0), (I, M, 5), (0, 1, 3), (1, M, 1), (2, 0, 5), (0, 2, 4), (0, 0, 0), (I, 0, 6), (0, 1, 6),
            (1, 0, 4), (0, 0, 1), (I, 2, 3)]


def _melee_multi(n, iz, mz, ms, **kw):
    return _abi.multi_env_config(n, "extermination", [], Map.from_text(MELEE_MAP, name="melee"), ["0", "1"],
                                 initial_zombies=iz, minimum_zombies=mz, agent_weapons=["shotgun", "rifle"],
                                 max_episode_steps=ms, observation_surroundings_width=7, **kw)


def _melee_single(n, iz, mz, ms, **kw):
    return _abi.single_env_config(n, "extermination", ["terminator"], Map.from_text(MELEE_MAP, name="melee"), 0,
                                  initial_zombies=iz, minimum_zombies=mz, observation_scope="surroundings:7",
                                  observation_position_encoding="channels", agent_weapon="shotgun", max_episode_steps=ms, **kw)


def _bridge(n, iz, mz, ms, **kw):
    return _abi.multi_env_config(n, "extermination", [], "bridge64", ["0", "1"], initial_zombies=iz, minimum_zombies=mz,
                                 max_episode_steps=ms, observation_surroundings_width=9, **kw)


# config -> (builder(n, initial, minimum, max_steps, **kw), caps (I, M, max_episode_steps), discrete actions)
CONFIGS = {"melee": (_melee_multi, (4, 3, 5), 7), "melee_single": (_melee_single, (4, 3, 5), 6), "bridge64": (_bridge, (6, 3, 5), 7)}


class Row(object):
    def __init__(self, G, kernel, defer, graph, config, seed0):
        self.G, self.kernel, self.defer, self.graph, self.config, self.seed0 = G, kernel, defer, graph, config, seed0
        self.make, self.caps, self.nd = CONFIGS[config]
        self.n = S.ENVS[G]
        launch, self.step_kernel, self.tick_waves = S.KERNEL_LAUNCH[kernel]
        self.launch = dict(launch, fobs=-1, defer_respawn=defer)
        self.id = "G%d-%s-%s-%s-%s@%d" % (G, kernel, "k_respawn" if defer > 0 else "tick", "graph" if graph else "eager",
                                          config, self.n)

    def seeds(self):
        return [self.seed0 + i for i in range(self.n)]

    def triples(self):
        t = TRIPLES(*self.caps[:2])
        return [t[e % len(t)] for e in range(self.n)]

    def changed(self):
        """Case 2: {env: its new triple} for every other env, the list walked from another start."""
        t = TRIPLES(*self.caps[:2])
        return {e: t[(e + 5) % len(t)] for e in range(0, self.n, 2)}

    def builder(self, env_params=True):
        """The engine's config: the caps, the row's G and launch overrides."""
        b = self.make(self.n, *self.caps, env_params=env_params)
        b.cfg.lanes_per_env = self.G
        return b.set_launch(self.launch)

    def oracle(self, triple):
        """One oracle env of the config an env with `triple` runs."""
        from oracle.oracle import OracleEnv
        return OracleEnv(self.make(1, *triple))

    def describe(self):
        return {"envs": self.n, "lanes_per_env": self.G, "step_kernel": self.step_kernel, "tick_waves": self.tick_waves,
                "respawn": "k_respawn" if self.defer > 0 else "tick", "env_params": 1}

    def actions(self, seeds, t, n_agents):
        return np.array([[A.DISCRETE_TRIPLES[A.discrete_action_id(s, t, a, self.nd)] for a in range(n_agents)]
                         for s in seeds], dtype=np.int32)


ROWS = [Row(1, "k_step", -1, False, "melee", 41000),
        Row(8, "k_tick5", 1, True, "melee", 42000),
        Row(16, "k_tick6", -1, True, "melee_single", 43000),
        Row(64, "k_step", 1, False, "bridge64", 44000),
        Row(16, "k_step", 1, False, "melee_single", 45000),
        Row(8, "k_step", -1, True, "melee", 46000),
        Row(64, "k_tick5", -1, True, "bridge64", 47000),
        Row(1, "k_tick6", 1, False, "melee", 48000)]
# the rows of case 2 (changed mid-run): both kernels, both respawn paths, eager and graphed, both surfaces
CHANGE_ROWS = [ROWS[1], ROWS[2], ROWS[3], ROWS[5]]
CLAIMS = ("timelimit", "respawn", "below", "win")


def n_zombies(state):
    return sum(1 for d in state["dyn"] if d[0] == _abi.THING_ZOMBIE)


class Track(object):
    """One env's oracle through a run with autoresets, and what the run shows of CLAIMS."""

    def __init__(self, row, seed, triple):
        self.row, self.seed, self.triple, self.pending = row, seed, triple, None
        self.o = row.oracle(triple)
        self.o.seed(seed)
        self.need, self.ep, self.seen = False, 0, set()
        self.low = False  # `below`: the zombies have numbered less than M in this episode, and never more since
        self.resp = 0

    def reset(self):
        if self.pending is not None:  # the env takes up its new triple: an oracle env of that config goes on with
            old, self.triple, self.pending = self.o, self.pending, None  # the stream and the obstacles' lives
            self.o = self.row.oracle(self.triple)
            self.o.set_rng(old.get_rng())
            for i, life, present in old.state()["obst"]:
                self.o.poke_obstacle(i, life)
                if not present:
                    self.o.poke_obstacle_gone(i)
            self.resp = 0
        self.need, self.ep, self.low = False, 0, False
        return self.o.reset()

    def step(self, t):
        """(obs, rewards or None for a reset, done, truncated, listed) of step t, as the engine's autoreset has it."""
        I, M = self.row.caps[:2]
        if self.need:
            return self.reset(), None, False, False, np.ones(self.o.A, bool)
        obs, r, d, tr, lb = self.o.step(self.row.actions([self.seed], t, self.o.A)[0])
        self.ep += 1
        self.need = d or tr
        iz, mz, ms = self.triple
        c = self.o.census()["respawns"]
        if c != self.resp and 0 < mz < M:
            self.seen.add("respawn")
        self.resp = c
        if tr and not d and ms > 0 and self.ep == ms:
            self.seen.add("timelimit")
        if d and iz < I and (r[:self.o.A][lb] >= 9.0).any():
            self.seen.add("win")
        if mz == 0 and iz >= 1:
            # overwritten at every step: True at the episode's (or the run's) end says the last step was below M,
            # which is the claim with "some step" read as the last one; with minimum_e = 0 nothing respawns, so the
            # count never rises and the flag, once up, stays up
            self.low = n_zombies(self.o.state()) < M
            if self.low and self.need:
                self.seen.add("below")
        return obs, r, d, tr, lb


def census(row, steps=STEPS, change=False):
    """The oracle alone over the row: claim -> the number of envs that show it."""
    tracks = [Track(row, s, tr) for s, tr in zip(row.seeds(), row.triples())]
    for k in tracks:
        k.reset()
    for t in range(1, steps + 1):
        if change and t == CHANGE_AFTER + 1:
            for e, tr in row.changed().items():
                tracks[e].pending = tr
        for k in tracks:
            k.step(t)
    got = {}
    for k in tracks:
        if k.low:  # still below at the run's end (an episode without a limit)
            k.seen.add("below")
        for c in k.seen:
            got[c] = got.get(c, 0) + 1
    return got


def run(row, change=False, steps=STEPS):
    """GPU: the row's engine (flagged, the per-env triples set before the first reset) against one oracle env per
    env at every step: the reset observation, then observations, rewards as float64 bits, done, truncated, listed,
    the autoreset flag, env_params(current=True), the full state with the slots past the env's own absent, and
    after the last step the RNG streams.  change: after step CHANGE_AFTER half the envs get another triple through
    an index tensor with check=False; an env keeps its current one until its next reset."""
    import torch
    from libzombsole_amd.engine import Engine
    from step_runner import GuardedStep

    eng = Engine(row.builder())
    desc = eng.describe()
    assert {k: desc[k] for k in row.describe()} == row.describe(), desc
    seeds, trip = row.seeds(), row.triples()
    eng.seed(seeds)
    n, Ag, P = row.n, eng.A, eng.builder.num_bots
    caps = torch.tensor([list(row.caps)] * n, dtype=torch.int32)
    assert torch.equal(eng.env_params().cpu(), caps) and torch.equal(eng.env_params(current=True).cpu(), caps)
    eng.set_env_params(torch.tensor(trip, dtype=torch.int32))
    assert eng.env_params().cpu().tolist() == [list(t) for t in trip]
    assert torch.equal(eng.env_params(current=True).cpu(), caps)  # until the reset
    tracks = [Track(row, s, t) for s, t in zip(seeds, trip)]
    obs0 = eng.reset().cpu().numpy()
    for k, tr in enumerate(tracks):
        assert np.array_equal(obs0[k], tr.reset()), ("reset obs", k)
    out = GuardedStep(eng)
    kinds = [o[2] for o in eng.builder.map.obstacles]
    resets = 0
    for t in range(1, steps + 1):
        if change and t == CHANGE_AFTER + 1:
            new = row.changed()
            idx = torch.tensor(sorted(new), dtype=torch.int32, device=eng.device)
            eng.set_env_params(torch.tensor([new[e] for e in sorted(new)], dtype=torch.int32, device=eng.device), envs=idx,
                               check=False)
            for e, v in new.items():
                tracks[e].pending = v
            assert eng.env_params().cpu().tolist() == [list(new.get(e, tracks[e].triple)) for e in range(n)]
        out.clear()
        if row.graph:
            eng.step_graph(t, row.nd, out=out, actions=out.actions)
        else:
            eng.gen_actions(t, row.nd, out=out.actions)
            eng.step(actions=out.actions, out=out)
        torch.cuda.synchronize()
        out.check(t)
        g = {k: getattr(out, k).cpu().numpy() for k in ("obs", "rewards", "done", "trunc", "listed", "was_reset", "actions")}
        assert np.array_equal(g["actions"], row.actions(seeds, t, Ag))
        cur = eng.env_params(current=True).cpu().tolist()
        for k, tr in enumerate(tracks):
            exp, r, d, trc, lb = tr.step(t)
            resets += r is None
            assert bool(g["was_reset"][k]) == (r is None), ("autoreset flag", k, t)
            assert bool(g["done"][k]) == d and bool(g["trunc"][k]) == trc, ("flags", k, t, tr.triple)
            assert np.array_equal(g["listed"][k].astype(bool), lb), ("listed", k, t)
            if r is None:
                assert not g["rewards"][k].any(), ("rewards of a reset", k, t)
            else:
                R = g["rewards"].shape[1]
                sel = lb if R == Ag else slice(0, 1)
                assert np.array_equal(g["rewards"][k][sel].view(np.uint64), r[:R][sel].view(np.uint64)), ("rew", k, t)
            assert np.array_equal(g["obs"][k], exp), ("obs", k, t, tr.triple)
            assert cur[k] == list(tr.triple), ("current triple", k, t, cur[k], tr.triple)
            st = eng.get_state(k)
            assert st.canonical(kinds) == tr.o.state(), ("state", k, t, tr.triple)
            assert not st.ent[Ag + P + max(tr.triple[0], tr.triple[1]):, 1].any(), ("a slot past the env's own", k, t)
    for k, tr in enumerate(tracks):
        assert np.array_equal(eng.get_rng(k), tr.o.get_rng()), ("rng stream", k)
    assert not eng.overflow() & _abi.OVF_PARAM_RANGE
    eng.close()
    return resets
