#!/usr/bin/env python3
"""Generate the entity-action fixtures (eact_*.json.gz) by running the REAL reference, like make_mask_golden.py, with
its configs (the mask_open and mask_strip maps and weapon mixes: every weapon, a bot, a dead agent, a lone agent, an
obstacle re-spawned destroyed) and golden_driver.run_config's records, unchanged (the existing replays compare them
key by key), and beside a run's `calls` its `probes`: per call and agent a list of [kind, dx, dy, ok].

A probe is computed by the reference itself, by make_mask_golden.py's method: the world is deep-copied, the copy of the
agent gets {"action_type": "attack" | "heal", "parameter": [dx, dy]} (set_action), its next_step must return an action,
World.execute_actions runs that one action on the copy (`random`'s state saved and restored around it) and the event it
logs must be a success ('injured', 'healed'; core.py:168-202).  The offsets probed are the four adjacent ones (empty
and out-of-map cells included) and the offset of every thing of World.things within distance 11 of the agent.  The
probes know nothing of slots or rows.  An agent that is not in World.things has no probes.

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_entity_act_golden.py
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
import make_mask_golden as MM  # noqa: E402  (the configs)

from golden_driver import run_config  # noqa: E402

SUCCESS = ("injured ", "healed ")
ADJACENT = ((0, 1), (-1, 0), (0, -1), (1, 0))
FAR2 = 11 * 11
KINDS = (("attack", 2), ("heal", 4))  # the action type and its ZS_ACT_* code
LOG = []

CONFIGS = [("eact_" + c[0][len("masks_"):],) + tuple(c[1:]) for c in MM.CONFIGS]


def reference_probes(game):
    world = game.world
    rows = []
    for agent in game.agents:
        row = []
        if world.things.get(agent.position) is agent:
            ax, ay = agent.position
            offsets = list(ADJACENT)
            for (x, y), t in world.things.items():
                d = (x - ax, y - ay)
                if t is not agent and d[0] ** 2 + d[1] ** 2 <= FAR2 and d not in offsets:
                    offsets.append(d)
            for name, code in KINDS:
                for dx, dy in offsets:
                    memo = {}
                    w2 = copy.deepcopy(world, memo)
                    a2 = memo[id(agent)]
                    a2.set_action({"action_type": name, "parameter": [dx, dy]})
                    nxt = a2.next_step(w2.things, w2.t)
                    ok = 0
                    if nxt is not None:
                        st = random.getstate()
                        n0 = len(w2.events)
                        w2.execute_actions([(a2, nxt[0], nxt[1])])
                        random.setstate(st)
                        ok = int(w2.events[n0][2].startswith(SUCCESS))
                    row.append([code, dx, dy, ok])
        rows.append(row)
    return rows


def probed(cls):
    class Probed(cls):
        def reset(self, *a, **kw):
            r = super().reset(*a, **kw)
            LOG.append(reference_probes(self.env.game))
            return r

        def step(self, *a, **kw):
            r = super().step(*a, **kw)
            LOG.append(reference_probes(self.env.game))
            return r
    return Probed


class K(MG.K):
    ZombsoleGymEnvDiscreteAction = probed(MG.K.ZombsoleGymEnvDiscreteAction)
    MultiagentZombsoleEnvDiscreteAction = probed(MG.K.MultiagentZombsoleEnvDiscreteAction)


def main():
    only = set(sys.argv[1:])
    for cfg in CONFIGS:
        if only and cfg[0] not in only:
            continue
        del LOG[:]
        data = run_config(cfg, K)
        it = iter(LOG)
        for run in data["runs"]:
            run["probes"] = [next(it) for _ in run["calls"]]
        assert next(it, None) is None, "one env call per record"
        path = os.path.join(HERE, cfg[0] + ".json.gz")
        with gzip.GzipFile(path, "wb", mtime=0) as f:
            f.write(json.dumps(data, separators=(",", ":")).encode("utf-8"))
        n = sum(len(r) for run in data["runs"] for call in run["probes"] for r in call)
        ok = sum(p[3] for run in data["runs"] for call in run["probes"] for r in call for p in r)
        print("%-40s %8d bytes %6d probes %6d ok" % (cfg[0], os.path.getsize(path), n, ok))


if __name__ == "__main__":
    main()
