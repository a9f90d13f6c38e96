#!/usr/bin/env python3
"""Generate the autopilot fixtures (pilot/pilot_*.json.gz) by running the REAL reference, like make_mask_golden.py and with
its driver: golden_driver.run_config's records over the non-discrete envs, and beside a run's `calls` its `pilot`: per
call, {"terminator" | "sniper" | "troll": [agent][3]}, the triple of each scripted policy for each agent.

The triples are the reference's own decisions.  At every call, for every agent in World.things, the reference's
Terminator, Sniper and Troll objects are built with the agent's weapon, position and life, their next_step(world.things,
world.t) is called and the (action, target) it returns is written as a triple by the rules of csrc/zs_autopilot.hpp.
Then the agent itself is given that triple's action dict (set_action) and its own next_step must return the same
(action, target): the same Thing, the same cell, or None.  That assertion is the reference proving that stepping an
agent with the triples is stepping the bot in its place; it holds on every call or the run stops.

A config's extras say how its steps are taken: "pilot": a policy name per agent (the step takes those triples, read
from the previous call's record), or "discrete": the bench's random discrete ids (so the states are not only the ones
the bots reach).  "poke_things": [[seed, call, rank, x, y], ...]: after that call of that seed's run, before anything of
it is recorded, the thing at `rank` of World.things' non-obstacle things (dict order) is moved to (x, y) as a move
does it (re-inserted last); the call's observation is the one from before the poke.  Every record carries extras
"views" (the zombies' idents, for pilot_census.py).

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_pilot_golden.py [--search N] [names...]
"""
import gzip
import json
import os
import random
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.dont_write_bytecode = True
sys.path.insert(0, HERE)
import make_golden as MG  # noqa: E402  (sets up the import path of the reference and its shims)

from golden_driver import run_config  # noqa: E402
import pilot_census  # noqa: E402
from libzombsole_amd import actions as A  # noqa: E402
from libzombsole_amd import autopilot as AP  # noqa: E402

from zombsole.players.terminator import Terminator  # noqa: E402
from zombsole.players.sniper import Sniper  # noqa: E402
from zombsole.players.troll import Troll  # noqa: E402

BOTS = {"terminator": Terminator, "sniper": Sniper, "troll": Troll}
CUR = {}  # the config being run: extras, the seeds still to come, the run's call counter, log and last record

# name, surface, stream, ctor kwargs, seeds, calls, full_obs_calls, max_steps, extras (make_golden.py's form)
CONFIGS = [
    # four weapons on the open 12 x 6 map without border walls, every agent a terminator; boxes 0 and 4 are re-spawned
    # destroyed at every reset and removed by the first cleanup
    ("pilot_multi_open_a4_weapons", "multi", "rich",
     dict(rules_name="extermination", player_names=[], map_name="mask_open", agent_ids=["0", "1", "2", "3"],
          initial_zombies=3, minimum_zombies=0, agent_weapons=["knife", "axe", "shotgun", "gun"]),
     [2, 5], 40, 1, 12, {"pilot": ["terminator"] * 4, "poke_obstacles": [[0, -5], [4, 0]], "views": True}),
    # knives and a troll bot among respawning zombies on the 7 x 3 strip, random discrete actions
    ("pilot_multi_strip_a2_knife_bot", "multi", "rich",
     dict(rules_name="survival", player_names=["troll"], map_name="mask_strip", agent_ids=["0", "1"],
          initial_zombies=3, minimum_zombies=3, agent_weapons="knife"),
     [0, 1], 40, 1, 0, {"pilot": "discrete", "views": True}),
    # a terminator, a sniper and a troll in the agents' slots, knives, on the open map
    ("pilot_multi_open_a3_mixed", "multi", "rich",
     dict(rules_name="extermination", player_names=[], map_name="mask_open", agent_ids=["0", "1", "2"],
          initial_zombies=4, minimum_zombies=0, agent_weapons=["knife", "shotgun", "knife"]),
     [1, 2], 40, 1, 14, {"pilot": ["terminator", "sniper", "troll"], "views": True}),
    ("pilot_multi_boxed_a2_knife", "multi", "rich",
     dict(rules_name="extermination", player_names=[], map_name="boxed", agent_ids=["0", "1"],
          initial_zombies=4, minimum_zombies=0, agent_weapons=["knife", "axe"]),
     [0, 1], 40, 1, 15, {"pilot": ["terminator"] * 2, "views": True}),
    ("pilot_multi_bridge_a3_discrete", "multi", "rich",
     dict(rules_name="extermination", player_names=["terminator"], map_name="bridge", agent_ids=["0", "1", "2"],
          initial_zombies=8, minimum_zombies=0, agent_weapons=["knife", "shotgun", "rifle"]),
     [1, 3], 40, 1, 13, {"pilot": "discrete", "views": True}),
    # a zombie put two cells outside the map's left border at the reset call: the best cell of an agent on that border
    # is outside the map
    ("pilot_multi_strip_a2_poked", "multi", "rich",
     dict(rules_name="extermination", player_names=[], map_name="mask_strip", agent_ids=["0", "1"],
          initial_zombies=1, minimum_zombies=0, agent_weapons="knife"),
     [0, 1], 40, 1, 11, {"pilot": ["terminator"] * 2, "poke_things": [[0, 0, 2, -2, 1], [1, 0, 2, -2, 1]], "views": True}),
    # the single surface, a knife, with a terminator bot beside it
    ("pilot_single_strip_bot", "single", "rich",
     dict(rules_name="extermination", player_names=["terminator"], map_name="mask_strip", agent_id=0,
          initial_zombies=2, minimum_zombies=0, observation_scope="world", observation_position_encoding="simple",
          agent_weapon="knife"),
     [0, 4], 40, 1, 9, {"pilot": ["terminator"], "views": True}),
]


def to_triple(agent, res, stand_in):
    """The triple of a bot's (action, target), by the rules of csrc/zs_autopilot.hpp."""
    if res is None:
        return None  # the policy's caller says what an idle bot's triple is
    action, target = res
    rel = (lambda q: [q[0] - agent.position[0], q[1] - agent.position[1]])
    if action == "move":
        return [A.ACT_MOVE] + rel(target)
    if action == "heal":
        return [A.ACT_HEAL, 0, 0] if target is stand_in else [A.ACT_HEAL] + rel(target.position)
    assert action == "attack"
    return [A.ACT_ATTACK_CLOSEST, 0, 0] if isinstance(target, MG.Zombie) else [A.ACT_ATTACK] + rel(target.position)


def same_decision(agent, bot, res, triple, world):
    """Agent.next_step on the triple's action dict returns what the bot returned."""
    keep = {k: getattr(agent, k, None) for k in ("action", "action_type", "action_parameter", "status")}
    agent.set_action(AP.to_action_dict(triple))
    got = agent.next_step(world.things, world.t)
    for k, v in keep.items():
        setattr(agent, k, v)
    if res is None or got is None:
        return res is None and got is None
    if res[0] != got[0]:
        return False
    if res[1] is bot:
        return got[1] is agent
    return got[1] is res[1] if not isinstance(res[1], tuple) else tuple(got[1]) == tuple(res[1])


def reference_pilot(game):
    world = game.world
    st = random.getstate()
    out = {name: [] for name in BOTS}
    for agent in game.agents:
        here = world.things.get(agent.position) is agent
        for name, cls in BOTS.items():
            if not here:
                out[name].append([A.ACT_IDLE, 0, 0])
                continue
            bot = cls(name, "cyan", position=agent.position, weapon=agent.weapon, rules=agent.rules,
                      objectives=agent.objectives)
            bot.life = agent.life
            res = bot.next_step(world.things, world.t)
            triple = to_triple(agent, res, bot)
            if triple is None:
                assert name == "sniper"
                triple = [A.ACT_ATTACK_CLOSEST, 0, 0]
            assert same_decision(agent, bot, res, triple, world), (name, res, triple, agent.position)
            out[name].append(triple)
    random.setstate(st)
    return out


def poke(game, rank, x, y):
    world = game.world
    dyn = [t for t in world.things.values() if not isinstance(t, (MG.Box, MG.Wall))]
    t = dyn[rank]
    assert (x, y) not in world.things
    del world.things[t.position]
    t.position = (x, y)
    world.things[t.position] = t


def piloted(cls, multi):
    class Piloted(cls):
        def __init__(self, *a, **kw):
            super().__init__(*a, **kw)
            CUR["seed"] = CUR["seeds"].pop(0)
            CUR["call"] = -1

        def _after(self):
            CUR["call"] += 1
            for seed, call, rank, x, y in CUR["extras"].get("poke_things", []):
                if (seed, call) == (CUR["seed"], CUR["call"]):
                    poke(self.game, rank, x, y)
            CUR["last"] = reference_pilot(self.game)
            CUR["log"].append((CUR["seed"], CUR["call"], CUR["last"]))

        def reset(self, *a, **kw):
            r = super().reset(*a, **kw)
            self._after()
            return r

        def step(self, act):
            ids = list(self.possible_agents) if multi else [None]
            how = CUR["extras"]["pilot"]
            mine = []
            for i, aid in enumerate(ids):
                if how == "discrete":
                    k = int(A.discrete_action_id(CUR["seed"], CUR["call"] + 1, i, 7 if multi else 6))
                    d = AP.to_action_dict(A.DISCRETE_TRIPLES[k])
                else:
                    d = AP.to_action_dict(CUR["last"][how[i]][i])
                mine.append(d)
            CUR["acts"].append(mine)
            r = super().step({aid: dict(d) for aid, d in zip(ids, mine)} if multi else dict(mine[0]))
            self._after()
            return r
    return Piloted


class K(MG.K):
    ZombsoleGymEnv = piloted(MG.K.ZombsoleGymEnv, False)
    MultiagentZombsoleEnv = piloted(MG.K.MultiagentZombsoleEnv, True)


def run(cfg, seeds=None):
    cfg = tuple(cfg[:4]) + (list(seeds or cfg[4]),) + tuple(cfg[5:])
    CUR.update(extras=cfg[8], seeds=list(cfg[4]), log=[], acts=[])
    data = run_config(cfg, K)
    # run_config resets once ahead of call 0 (recorded as call 0); an env that ended is reset inside its next call
    log, acts = iter(CUR["log"]), iter(CUR["acts"])
    for r in data["runs"]:
        r["pilot"] = []
        for c, rec in enumerate(r["calls"]):
            seed, call, pl = next(log)
            assert (seed, call) == (r["seed"], c), (seed, call, r["seed"], c)
            r["pilot"].append(pl)
            if rec["kind"] == "step":  # the action the step took, not the one run_config generated
                mine = next(acts)
                rec["act"] = mine if data["surface"] == "multi" else mine[0]
    assert next(log, None) is None and next(acts, None) is None, "one env call per record"
    return data


def main():
    args = sys.argv[1:]
    search = 0
    if args[:1] == ["--search"]:
        search, args = int(args[1]), args[2:]
    only = set(args)
    total = None
    for cfg in CONFIGS:
        if only and cfg[0] not in only:
            continue
        if search:
            for seed in range(search):
                got = pilot_census.census(run(cfg, [seed]))
                print(cfg[0], seed, {k: got[k] for k in pilot_census.NEED if got[k]})
            continue
        data = run(cfg)
        path = os.path.join(HERE, "pilot", cfg[0] + ".json.gz")
        with gzip.GzipFile(path, "wb", mtime=0) as f:
            f.write(json.dumps(data, separators=(",", ":")).encode("utf-8"))
        total = pilot_census.census(data, total)
        print("%-40s %8d bytes" % (cfg[0], os.path.getsize(path)))
    if total is not None:
        for k in sorted(total):
            print("  %-36s %d" % (k, total[k]))
        print("missing:", pilot_census.missing(total))


if __name__ == "__main__":
    main()
