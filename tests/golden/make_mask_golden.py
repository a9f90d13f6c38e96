#!/usr/bin/env python3
"""Generate the action-mask fixtures (masks_*.json.gz) by running the REAL reference, like make_golden.py and with
its driver: golden_driver.run_config's records, unchanged (the existing replays compare them key by key), and beside
a run's `calls` its `masks`: per call, [agent][8] of 0/1.

Bit k of agent a is computed by the reference itself: the world is deep-copied, the copy of the agent gets
game_actions[k] (set_action), its next_step must return an action, World.execute_actions runs that one action on
the copy (`random`'s state saved and restored around it) and the event it logs must be a success ('moved to',
'injured', 'healed'; core.py:140-202).  An agent that is not in World.things gets zeros.

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_mask_golden.py
"""
import copy
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
import mask_census  # noqa: E402

SUCCESS = ("moved to ", "injured ", "healed ")
LOG = []

# name, surface, stream, ctor kwargs, seeds, calls, full_obs_calls, max_steps, extras (make_golden.py's form)
CONFIGS = [
    # four weapons on the open 12 x 6 map (no border walls: agents spawn in the corners and on the left border);
    # boxes 0 and 4 are re-spawned destroyed at every reset and removed by the first cleanup
    ("masks_multi_open_a4_weapons", "multi", "discrete",
     dict(rules_name="extermination", player_names=[], map_name="mask_open", agent_ids=["0", "1", "2", "3"],
          initial_zombies=3, minimum_zombies=0, agent_weapons=["knife", "axe", "shotgun", "gun"]),
     [0, 1], 40, 1, 12, {"poke_obstacles": [[0, -5], [4, 0]]}),
    # rifles, a bot to heal, zombies enough to kill agents: a dead agent beside a live one, a lone agent
    ("masks_multi_open_a2_rifle_bot", "multi", "discrete",
     dict(rules_name="survival", player_names=["terminator"], map_name="mask_open", agent_ids=["0", "1"],
          initial_zombies=8, minimum_zombies=8), [0, 1], 40, 1, 0),
    ("masks_multi_open_a3_rifle_sparse", "multi", "discrete",
     dict(rules_name="extermination", player_names=[], map_name="mask_open", agent_ids=["0", "1", "2"],
          initial_zombies=1, minimum_zombies=0), [0, 1], 40, 1, 10),
    # knives among respawning zombies on the 7 x 3 strip: one agent outlives the other (a lone agent heals itself)
    ("masks_multi_strip_a2_knife", "multi", "discrete",
     dict(rules_name="survival", player_names=[], map_name="mask_strip", agent_ids=["0", "1"],
          initial_zombies=4, minimum_zombies=4, agent_weapons="knife"), [0, 1], 40, 1, 0),
    # the single surface (six ids) on the 7 x 3 strip, with a bot
    ("masks_single_strip_bot", "single", "discrete",
     dict(rules_name="extermination", player_names=["terminator"], map_name="mask_strip", agent_id=0,
          initial_zombies=2, minimum_zombies=0, observation_scope="world",
          observation_position_encoding="simple"), [0, 1], 40, 1, 9,
     {"poke_obstacles": [[1, -3]]}),
]


def reference_masks(game, game_actions):
    world = game.world
    rows = []
    for agent in game.agents:
        row = [0] * 8
        if world.things.get(agent.position) is agent:
            for k, act in enumerate(game_actions):
                memo = {}
                w2 = copy.deepcopy(world, memo)
                a2 = memo[id(agent)]
                a2.set_action(copy.deepcopy(act))
                nxt = a2.next_step(w2.things, w2.t)
                if nxt is None:
                    continue
                st = random.getstate()
                n0 = len(w2.events)
                w2.execute_actions([(a2, nxt[0], nxt[1])])
                random.setstate(st)
                row[k] = int(w2.events[n0][2].startswith(SUCCESS))
        rows.append(row)
    return rows


def masked(cls):
    class Masked(cls):
        def reset(self, *a, **kw):
            r = super().reset(*a, **kw)
            LOG.append(reference_masks(self.env.game, self.game_actions))
            return r

        def step(self, *a, **kw):
            r = super().step(*a, **kw)
            LOG.append(reference_masks(self.env.game, self.game_actions))
            return r
    return Masked


class K(MG.K):
    ZombsoleGymEnvDiscreteAction = masked(MG.K.ZombsoleGymEnvDiscreteAction)
    MultiagentZombsoleEnvDiscreteAction = masked(MG.K.MultiagentZombsoleEnvDiscreteAction)


def main():
    only = set(sys.argv[1:])
    total = None
    for cfg in CONFIGS:
        if only and cfg[0] not in only:
            continue
        del LOG[:]
        data = run_config(cfg, K)
        it = iter(LOG)
        for run in data["runs"]:
            run["masks"] = [next(it) for _ in run["calls"]]
        assert next(it, None) is None, "one env call per record"
        path = os.path.join(HERE, cfg[0] + ".json.gz")
        with gzip.GzipFile(path, "wb", mtime=0) as f:
            f.write(json.dumps(data, separators=(",", ":")).encode("utf-8"))
        total = mask_census.census(data, total)
        print("%-40s %8d bytes" % (cfg[0], os.path.getsize(path)))
    for k in sorted(total):
        print("  %-36s %d" % (k, total[k]))
    print("missing:", mask_census.missing(total))


if __name__ == "__main__":
    main()
