#!/usr/bin/env python3
"""Generate golden vectors by running the REAL reference (this container only).

The reference (`/root/reference/zombsole`, pure Python) is imported read-only with
the no-op shims in ./shims for gymnasium / termcolor / cv2, which are absent from
this image and touch no game arithmetic.  Nothing of the
reference is copied: only its observable outputs are written, as JSON fixtures
under tests/golden/*.json.gz.

Parity protocol: for env seed s the reference is driven as
``random.seed(s); env.reset()`` followed by the counter-based action stream of
``libzombsole_amd.actions``.  After a step that returns done/truncated, the next
call is ``env.reset()`` *without* reseeding (the engine's next-step autoreset).
A `max_steps` config emulates gymnasium's TimeLimit (truncated once the episode
has taken that many steps), as registered in `zombsole/gym_env.py:382-414`.

Recorded per call: obs sha256 (full obs for the first calls), rewards as float
hex, done/truncated, and a canonical state dump (dynamic things in dict order,
changed obstacles, dead-body cells, counters, agent/bot records).

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden.py
"""
import gzip
import hashlib
import json
import os
import random
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.abspath(os.path.join(HERE, "..", ".."))
REF = "/root/reference"
sys.dont_write_bytecode = True
sys.path.insert(0, os.path.join(HERE, "shims"))
sys.path.insert(0, REF)
sys.path.insert(0, REPO)

sys.path.insert(0, os.path.join(REPO, "tests"))
from golden_driver import run_config  # noqa: E402

from zombsole.things import Box, Wall, Zombie, Player, DeadBody  # noqa: E402
from zombsole.players.agent import Agent  # noqa: E402
from zombsole.gym_env import ZombsoleGymEnv, ZombsoleGymEnvDiscreteAction  # noqa: E402
from zombsole.gym.multiagent_env import (  # noqa: E402
    MultiagentZombsoleEnv, MultiagentZombsoleEnvDiscreteAction)

SYN = os.path.join(REPO, "libzombsole_amd", "maps")


def map_arg(name):
    if name in ("bridge64", "city128"):
        return os.path.join(SYN, name + ".txt")
    test_map = os.path.join(HERE, "maps", name + ".txt")  # test-only maps (absolute path, gym_env.py:55)
    if os.path.isfile(test_map):
        return test_map
    return name


# name, surface, stream, ctor kwargs, seeds, calls, full_obs_calls, max_steps
CONFIGS = [
    ("single_bridge_world_simple", "single", "discrete",
     dict(rules_name="extermination", player_names=[], map_name="bridge", agent_id=0,
          initial_zombies=10, minimum_zombies=0, observation_scope="world",
          observation_position_encoding="simple"), [0, 1, 2], 160, 2, 0),
    ("single_bridge_surr21_terminator_rich", "single", "rich",
     dict(rules_name="extermination", player_names=["terminator"], map_name="bridge",
          agent_id=0, initial_zombies=10, minimum_zombies=3,
          observation_scope="surroundings:21", observation_position_encoding="simple"),
     [3, 4], 160, 2, 60),
    ("single_boxed_world_channels_bots_rich", "single", "rich",
     dict(rules_name="extermination", player_names=["terminator", "sniper", "troll"],
          map_name="boxed", agent_id=0, initial_zombies=1, minimum_zombies=1,
          observation_scope="world", observation_position_encoding="channels",
          agent_weapon="shotgun"), [5, 6], 120, 2, 40),
    ("single_easyexit_survival_rngbots_rich", "single", "rich",
     dict(rules_name="survival", player_names=["hamster", "randoman", "troll"],
          map_name="easy_exit", agent_id="0", initial_zombies=6, minimum_zombies=4,
          observation_scope="surroundings:7", observation_position_encoding="channels",
          agent_weapon="random"), [7, 8], 150, 2, 50),
    ("multi_bridge64_a2_z10", "multi", "discrete",
     dict(rules_name="extermination", player_names=[], map_name="bridge64",
          agent_ids=["0", "1"], initial_zombies=10, minimum_zombies=0),
     [0, 1, 2], 200, 2, 0),
    ("multi_boxed_a2_rich", "multi", "rich",
     dict(rules_name="extermination", player_names=[], map_name="boxed",
          agent_ids=["0", "1"], initial_zombies=1, minimum_zombies=0),
     [9, 10], 120, 2, 30),
    ("multi_bridge_a4_z20_evac_weapons", "multi", "rich",
     dict(rules_name="evacuation", player_names=["terminator"], map_name="bridge",
          agent_ids=["0", "1", "2", "3"], initial_zombies=20, minimum_zombies=5,
          agent_weapons=["random", "knife", "axe", "gun"]), [11, 12], 120, 2, 0),
    ("multi_fort_a32_z100", "multi", "discrete",
     dict(rules_name="extermination", player_names=[], map_name="fort",
          agent_ids=[str(i) for i in range(32)], initial_zombies=100, minimum_zombies=0),
     [13], 40, 1, 0),
    ("multi_cityfs_safehouse_a4_z50", "multi", "discrete",
     dict(rules_name="safehouse", player_names=[], map_name="city_for_safehouse",
          agent_ids=["0", "1", "2", "3"], initial_zombies=50, minimum_zombies=50),
     [14], 30, 1, 0),
    ("multi_city128_safehouse_a4_z50", "multi", "discrete",
     dict(rules_name="safehouse", player_names=[], map_name="city128",
          agent_ids=["0", "1", "2", "3"], initial_zombies=50, minimum_zombies=50),
     [15], 25, 1, 0),
    ("multi_hallway_survival_a3_rich", "multi", "rich",
     dict(rules_name="survival", player_names=["sniper"], map_name="hallway",
          agent_ids=["0", "1", "2"], initial_zombies=4, minimum_zombies=4,
          observation_surroundings_width=9), [16, 17], 120, 2, 40),
    ("multi_closet_safehouse_a2_rich", "multi", "rich",
     dict(rules_name="safehouse", player_names=[], map_name="to_the_closet",
          agent_ids=["0", "1"], initial_zombies=8, minimum_zombies=8,
          agent_weapons="shotgun"), [18], 120, 2, 0),
    # debug=True with parameters Agent.next_step raises on (actions.bad_action): World.step re-raises
    # after t += 1 and the earlier actors' decisions, incl. hamster / randoman RNG draws (core.py:72-99)
    ("single_easyexit_debug_badactions", "single", "bad",
     dict(rules_name="survival", player_names=["hamster", "randoman", "troll"], map_name="easy_exit",
          agent_id=0, initial_zombies=6, minimum_zombies=4, observation_scope="surroundings:7",
          observation_position_encoding="channels", agent_weapon="random", debug=True), [21, 22], 120, 2, 50),
    ("multi_bridge_debug_badactions_a3", "multi", "bad",
     dict(rules_name="extermination", player_names=["hamster", "randoman"], map_name="bridge",
          agent_ids=["0", "1", "2"], initial_zombies=10, minimum_zombies=4,
          observation_surroundings_width=11, debug=True), [23, 24], 120, 2, 60),
    # obstacle life carried over resets without a floor (game.py:151-155, core.py:72-78,168-184): walls
    # poked near the int16 floor are re-spawned destroyed at every reset and shot again on tick 1 by
    # rifle agents (two of them on the centre wall when the spawn shuffle puts them either side of it);
    # no zombies, so Extermination ends every episode after one step
    ("multi_wallhp_carryover_a2", "multi", "fixed",
     dict(rules_name="extermination", player_names=[], map_name="wall_hp", agent_ids=["0", "1"],
          initial_zombies=0, minimum_zombies=0), [25, 26, 27], 80, 4, 0,
     {"poke_obstacles": [[5, -32700], [6, -32720], [7, -32760]],
      "actions": [{"action_type": "attack", "parameter": [1, 0]},
                  {"action_type": "attack", "parameter": [-1, 0]}]}),
    # env.game views (golden_driver.ViewTracker): World.decoration in insertion order (bodies over
    # objectives and over earlier bodies), zombie identity across respawns, the values a removed zombie
    # keeps; respawns under a minimum count reuse the dead zombies' slots in the same step
    ("views_multi_bridge_a4_z20_respawn", "multi", "rich",
     dict(rules_name="extermination", player_names=["terminator"], map_name="bridge",
          agent_ids=["0", "1", "2", "3"], initial_zombies=20, minimum_zombies=15,
          agent_weapons=["shotgun", "rifle", "axe", "gun"]), [31, 32], 150, 1, 0, {"views": True}),
    ("views_single_fort_safehouse", "single", "rich",
     dict(rules_name="safehouse", player_names=["terminator", "sniper"], map_name="fort", agent_id=0,
          initial_zombies=30, minimum_zombies=30, observation_scope="surroundings:11",
          observation_position_encoding="channels", agent_weapon="shotgun"), [33], 150, 1, 60, {"views": True}),
    # World.events (core.py:68-70): idle actors, every executed action's message (moves out of bounds, into
    # things, too fast; attacks and heals in and out of range) and deaths, per step.  The rich stream gives
    # agents moves of any length, attacks and heals at any cell; the bots of the single-agent config draw in
    # their decisions (the leader's serial execution), the fort config crowds 40 zombies around 8 agents
    # (the lanes' chunked execution)
    ("events_multi_bridge_a4_rich", "multi", "rich",
     dict(rules_name="extermination", player_names=["terminator"], map_name="bridge",
          agent_ids=["0", "1", "2", "3"], initial_zombies=15, minimum_zombies=10,
          agent_weapons=["shotgun", "rifle", "knife", "gun"]), [41, 42], 100, 1, 0, {"events": True}),
    ("events_single_boxed_bots_rich", "single", "rich",
     dict(rules_name="extermination", player_names=["terminator", "sniper", "troll", "hamster"],
          map_name="boxed", agent_id=0, initial_zombies=2, minimum_zombies=2, observation_scope="world",
          observation_position_encoding="simple", agent_weapon="axe"), [43, 44], 120, 1, 40, {"events": True}),
    ("events_multi_fort_a8_z40", "multi", "discrete",
     dict(rules_name="extermination", player_names=[], map_name="fort",
          agent_ids=[str(i) for i in range(8)], initial_zombies=40, minimum_zombies=20), [45], 60, 1, 0,
     {"events": True}),
    # C1 (BASELINE.json configs[0]): the real bridge, extermination, agents ["0", "1"], 10 zombies, through
    # MultiagentZombsoleEnv(DiscreteAction) — the uniform Discrete(7) stream and the rich dict stream
    ("multi_bridge_a2_z10", "multi", "discrete",
     dict(rules_name="extermination", player_names=[], map_name="bridge",
          agent_ids=["0", "1"], initial_zombies=10, minimum_zombies=0), [0, 1, 2], 200, 2, 0),
    ("multi_bridge_a2_z10_rich", "multi", "rich",
     dict(rules_name="extermination", player_names=[], map_name="bridge",
          agent_ids=["0", "1"], initial_zombies=10, minimum_zombies=0), [3, 4], 150, 2, 0, {"events": True}),
    # next_step errors in World.events (core.py:96-99): without debug the agent's error is logged in place of
    # 'idle' and the step goes on; with debug the actors before it are logged, then its error, and the step
    # stops (that step's events land in the next recorded step's slice of the log)
    ("events_multi_bridge_a3_bad", "multi", "bad",
     dict(rules_name="extermination", player_names=["terminator"], map_name="bridge",
          agent_ids=["0", "1", "2"], initial_zombies=10, minimum_zombies=5), [51, 52], 100, 1, 0,
     {"events": True}),
    ("events_single_easyexit_debug_bad", "single", "bad",
     dict(rules_name="survival", player_names=["hamster", "randoman", "troll"], map_name="easy_exit",
          agent_id=0, initial_zombies=6, minimum_zombies=4, observation_scope="surroundings:7",
          observation_position_encoding="channels", agent_weapon="random", debug=True), [53], 120, 1, 50,
     {"events": True}),
    # The ways an episode ends (tests/outcomes.py; test_golden_outcomes.py counts them in the fixture files), on
    # the small maps of ./maps, 40 calls a seed.  The seeds are the first under which the reference's run holds
    # the outcomes named here.
    # safehouse won (every alive player on an objective), once on the step the TimeLimit truncates
    ("term_safe_tiny_a2", "multi", "discrete",
     dict(rules_name="safehouse", player_names=[], map_name="safe_tiny", agent_ids=["0", "1"],
          initial_zombies=3, minimum_zombies=3), [0, 3], 40, 1, 6),
    # safehouse won on the step the player off the objectives dies; safehouse lost
    ("term_safe_crowd_a2", "multi", "discrete",
     dict(rules_name="safehouse", player_names=[], map_name="safe_crowd", agent_ids=["0", "1"],
          initial_zombies=4, minimum_zombies=4), [0, 4], 40, 1, 0),
    # evacuation: the spawns touch only diagonally (not together); agents only, and with a bot (the walk over
    # the alive players starts from the first alive bot)
    ("term_evac_tiny_a4", "multi", "discrete",
     dict(rules_name="evacuation", player_names=[], map_name="evac_tiny", agent_ids=["0", "1", "2", "3"],
          initial_zombies=2, minimum_zombies=2), [0, 1], 40, 1, 6),
    ("term_evac_tiny_bot_a2", "multi", "discrete",
     dict(rules_name="evacuation", player_names=["terminator"], map_name="evac_tiny", agent_ids=["0", "1"],
          initial_zombies=2, minimum_zombies=2), [0, 1], 40, 1, 6),
    # evacuation among nine zombies with knives: lost with fewer than half alive; won with a dead member
    ("term_evac_crowd_a4", "multi", "discrete",
     dict(rules_name="evacuation", player_names=[], map_name="evac_crowd", agent_ids=["0", "1", "2", "3"],
          initial_zombies=9, minimum_zombies=9, agent_weapons="knife"), [0, 1], 40, 1, 0),
    # survival lost (every player dead) on both surfaces; the single one also truncates with the agent dead
    # and the troll alive
    ("term_surv_melee_a2", "multi", "discrete",
     dict(rules_name="survival", player_names=[], map_name="melee", agent_ids=["0", "1"],
          initial_zombies=14, minimum_zombies=14), [0, 1], 40, 1, 0),
    ("term_surv_single_troll", "single", "discrete",
     dict(rules_name="survival", player_names=["troll"], map_name="melee", agent_id=0, initial_zombies=14,
          minimum_zombies=14, observation_scope="surroundings:7", observation_position_encoding="channels"),
     [0, 1], 40, 1, 0),
    # extermination with a minimum of one zombie and one zombie spawn cell: the last zombie dies and the
    # respawn places one (the cell is free: the episode goes on) or none (an agent stands on it: won)
    ("term_ext_one_spawn_a2", "multi", "discrete",
     dict(rules_name="extermination", player_names=[], map_name="one_spawn", agent_ids=["0", "1"],
          initial_zombies=1, minimum_zombies=1, agent_weapons="axe"), [0, 3], 40, 1, 8),
]


class K:
    """The reference's classes, for golden_driver.run_config."""
    Box, Wall, Zombie, Player, DeadBody, Agent = Box, Wall, Zombie, Player, DeadBody, Agent
    ZombsoleGymEnv, ZombsoleGymEnvDiscreteAction = ZombsoleGymEnv, ZombsoleGymEnvDiscreteAction
    MultiagentZombsoleEnv = MultiagentZombsoleEnv
    MultiagentZombsoleEnvDiscreteAction = MultiagentZombsoleEnvDiscreteAction
    map_arg = staticmethod(map_arg)


def kw_for_fixture(cfg):
    kw = dict(cfg[3])
    return kw


def main():
    only = set(sys.argv[1:])
    for cfg in CONFIGS:
        if only and cfg[0] not in only:
            continue
        t0 = time.time()
        data = run_config(cfg, K)
        path = os.path.join(HERE, cfg[0] + ".json.gz")
        with gzip.open(path, "wt", encoding="utf-8") as f:
            json.dump(data, f, separators=(",", ":"))
        print("%-45s %6.1fs %8d bytes" % (cfg[0], time.time() - t0, os.path.getsize(path)))


if __name__ == "__main__":
    main()
