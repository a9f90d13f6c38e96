"""The shapes at which the reset and respawn work branches: k_reset (zs_reset.hpp reset_env_wave), k_respawn
(respawn_env_wave), their shared wave_spawn, and the tick leader's spawn_in_random (zs_tick.hpp).  None of these
is a template, but each branches on the shape of the config; every row below is the smallest config that reaches
one such branch, with the launch overrides (VARIANTS) under which it runs.  test_reset_shapes_plan.py checks on the
CPU that the compiled step plan resolves every row and variant to what the variant names and that the oracle's own
run of the row meets the events the row claims; test_reset_shapes.py runs every row and variant on the GPU against
the oracle; test_enospace.py runs the rows whose reset fails.

Maps are built here (field()): W x H cells, the player spawn list the first `nps` free cells in row-major order,
the zombie spawn list the last `nzs` ones from the bottom right backwards (0 = the map lists none: every cell).

Branches and their rows:
  * weapon picks of reset_env_wave: one lane per player for A + P <= 64 with the bots mask's A + P == 64 case
    (p63, p64), the serial lane-0 path above (p65, p100, single65), no random pick at all (nrw0); random picks are
    ranked bots first, then agents, so agents mix fixed and random weapons and the bots are of all five types
    (terminator and sniper bring their weapon, the others draw one);
  * entity rows: E = 64, 65 (respawn_env_wave's min(lane, E - 1) rows and its loop from slot 64) and 254;
  * zombie spawn lists of 0 (every cell, W * H no multiple of 64), 1, 64, 65, 512, 513 and 600 entries
    (respawn_env_wave's 8 x 64 registers and its tail loop from entry 512), each by k_respawn and by the tick's
    leader, fused and unfused, the lists in LDS; z600 also with the tick's candidate list in LDS and in HBM
    (cand_cap, read from the plan);
  * the lists read from HBM (hbm0, hbm1, hbm65, hbm512, hbm513, hbm600).  zs_launch.reset_lists = -1 does not reach that path by itself: it
    only keeps k_reset from staging more than the tick does, and the tick stages every list that fits its image
    (test_reset_shapes_plan.py pins that).  The rows take more than 4 096 list entries in all, which the plan
    never stages;
  * player spawn lists of exactly the players (every cell popped), one more, and one fewer (FAIL_ROWS);
  * short of room: fewer free zombie cells than the deficit at every respawn (short), a walled-in single cell that
    stays taken (z1: n = 0 and n = 1);
  * more than 4 096 obstacles (walls4200): the obstacle-present words from word 128 on.
"""
from libzombsole_amd import _abi
from libzombsole_amd import actions as A
from libzombsole_amd.maps import Map

import numpy as np

from stream_util import same_stream  # noqa: F401  (the tests of the table compare streams with it)

BOTS5 = ["hamster", "terminator", "troll", "sniper", "randoman"]
WEAPONS7 = ["random", "axe", "random", "gun", "rifle", "random", "knife"]
EPISODE = 4


def field(W, H, nps, nzs, walls=(), name="field"):
    """A W x H map: `walls` cells (x, y) in the given order, the first nps free cells (row-major) the player spawn
    list, the last nzs free cells (row-major, backwards) the zombie spawn list."""
    taken = set(walls)
    free = [(x, y) for y in range(H) for x in range(W) if (x, y) not in taken]
    assert nps + nzs <= len(free), (nps, nzs, len(free))
    m = Map((W, H), [(x, y, _abi.THING_WALL) for x, y in walls], free[:nps], free[::-1][:nzs], [], name=name)
    return m


def bots(n):
    return [BOTS5[i % 5] for i in range(n)]


def multi(n, m, agents, bot_names, initial, minimum, weapons=None, rules="survival", episode=EPISODE):
    return _abi.multi_env_config(n, rules, bot_names, m, [str(i) for i in range(agents)], initial_zombies=initial,
                                 minimum_zombies=minimum, observation_surroundings_width=5,
                                 agent_weapons=weapons or [WEAPONS7[i % 7] for i in range(agents)],
                                 max_episode_steps=episode)


# -- the maps ------------------------------------------------------------------------------------------------------
def yard(nps, nzs):
    """24 x 12 = 288 cells, 4.5 bitmap-ballot rounds of 64."""
    return field(24, 12, nps, nzs, name="yard")


def plain(nps, nzs):
    """40 x 18 = 720 cells (11.25 rounds of 64)."""
    return field(40, 18, nps, nzs, name="plain")


def niche_map():
    """12 x 6 with one zombie spawn cell walled in at the far corner: a zombie placed there never leaves it."""
    walls = [(9, 3), (10, 3), (11, 3), (9, 4), (9, 5), (10, 5), (11, 5), (11, 4)]
    m = field(12, 6, 6, 0, walls, name="niche")
    m.zombie_spawns = [(10, 4)]
    return m


N_WALLS, WALL_W, WALL_H = 4200, 96, 64


def walls_map():
    """96 x 64 with 4 200 walls: rows 10 .. 53 (4 224 cells) but the last 24; the zombie spawn list is the cells of
    the walls of index 4 096 and above (present-word 128 on), so zombies spawn only where a wall has gone."""
    cells = [(x, y) for y in range(10, 54) for x in range(WALL_W)][:N_WALLS]
    m = field(WALL_W, WALL_H, 8, 0, cells, name="walls4200")
    m.zombie_spawns = cells[4096:]
    return m


# -- the rows ------------------------------------------------------------------------------------------------------
# launch variants: name -> overrides ("lanes_per_env" is zs_config's field, the others zs_launch's)
V_FUSED = ("fused", {"fused": 1})
V_UNFUSED = ("k_reset", {"fused": -1})


def v_respawn(defer):
    tag = "k_respawn" if defer > 0 else "leader"
    return [(tag, {"fused": -1, "defer_respawn": defer}), (tag + "_fused", {"fused": 1, "defer_respawn": defer})]


V_BOTH = v_respawn(1) + v_respawn(-1)
# zs_launch.reset_lists = -1 as the engine takes it: the reset work stages no more than the tick does (with the tick's
# lists in LDS it reads them there, see test_reset_shapes_plan.py; on an hbm row nothing is staged either way)
V_LISTS_OFF = ("k_respawn_lists_off", {"fused": -1, "defer_respawn": 1, "reset_lists": -1})


class Row(object):
    """make(n) -> the config; claims: the oracle census counters (oracle.CENSUS_EXT, or "autoresets") that must be
    non-zero over the row's run; zero: those that must be zero; setup: "walls" marks the obstacles from index
    4 096 on as gone after the first reset."""

    def __init__(self, rid, make, n, steps, variants, claims, zero=(), setup=None):
        self.id, self.make, self.n, self.steps, self.variants = rid, make, n, steps, list(variants)
        self.claims, self.zero, self.setup = tuple(claims), tuple(zero), setup
        self.seed0 = None  # 4000 + 100 * the row's place in ROWS + FAIL_ROWS (set below the tables)

    def seeds(self):
        return [self.seed0 + i for i in range(self.n)]

    def builder(self, overrides=None, n=None):
        b = self.make(self.n if n is None else n)
        ov = dict(overrides or {})
        b.cfg.lanes_per_env = ov.pop("lanes_per_env", 0)
        return b.set_launch(dict(ov, fobs=-1) if overrides is not None else None)

    def actions(self, seeds, t, n_agents):
        """zs_gen_actions' stream at step t: int32 [len(seeds)][n_agents][3]."""
        return np.array([[A.DISCRETE_TRIPLES[A.discrete_action_id(s, t, a, 7)] for a in range(n_agents)]
                         for s in seeds], dtype=np.int32)


def _players(agents, nbots):
    # player spawns: 20 more cells than players; 6 zombies kept at 8 (a respawn at every episode's first step)
    return lambda n: multi(n, yard(agents + nbots + 20, 40), agents, bots(nbots), 6, 8)


def _single65(n):
    return _abi.single_env_config(n, "extermination", bots(64), yard(90, 40), 0, initial_zombies=6,
                                  minimum_zombies=8, agent_weapon="random", max_episode_steps=EPISODE)


def _zlist(nzs, initial=3, minimum=6):
    m = (lambda: plain(12, nzs)) if nzs > 200 else (lambda: yard(12, nzs))
    return lambda n: multi(n, m(), 2, ["hamster", "sniper"], initial, minimum, weapons=["shotgun", "random"])


def _hbm(nzs):
    """More than 4 096 spawn-list entries in all (a player spawn list of 4 100 cells): the plan stages no list in
    LDS, neither the tick's (lists_cap 0) nor the reset work's (rlists_cap 0)."""
    return lambda n: multi(n, field(96, 64, 4100, nzs, name="wide"), 2, ["hamster", "sniper"], 3, 6,
                           weapons=["shotgun", "random"])


def _entities(E, initial_short=2):
    z = E - 4
    return lambda n: multi(n, plain(12, 0 if E == 65 else 400), 2, ["terminator", "troll"], z - initial_short, z,
                           weapons=["shotgun", "rifle"])


def _pspawn(extra):
    """3 agents and 4 bots over 7 + extra player spawn cells."""
    return lambda n: multi(n, yard(7 + extra, 30), 3, bots(4), 3, 0, rules="extermination")


ROWS = [
    # players
    Row("p63", _players(7, 56), 7, 12, [V_FUSED, V_UNFUSED], ("autoresets", "respawns")),
    Row("p64", _players(7, 57), 7, 12, [V_FUSED, V_UNFUSED], ("autoresets", "respawns")),
    Row("p65", _players(7, 58), 7, 12, [V_FUSED, V_UNFUSED], ("autoresets", "respawns")),
    Row("p100", _players(9, 91), 5, 12, [V_FUSED, V_UNFUSED], ("autoresets", "respawns")),
    Row("nrw0", lambda n: multi(n, yard(10, 40), 2, ["terminator", "sniper", "sniper"], 4, 4,
                                weapons=["gun", "axe"]), 13, 12, [V_FUSED, V_UNFUSED], ("autoresets",)),
    Row("single65", _single65, 7, 12, [V_FUSED, V_UNFUSED], ("autoresets", "respawns")),
    # entities
    Row("e64", _entities(64), 7, 12, V_BOTH, ("autoresets", "respawns")),
    Row("e65", _entities(65), 7, 12, V_BOTH, ("autoresets", "respawns")),
    Row("e254", _entities(254, 10), 5, 12, v_respawn(1) + v_respawn(-1)[:1], ("autoresets", "respawns")),
    Row("init_only", lambda n: multi(n, yard(12, 40), 2, ["troll"], 6, 0), 13, 12, [V_FUSED, V_UNFUSED],
        ("autoresets",), zero=("respawns",)),
    # zombie spawn lists
    Row("z0", _zlist(0), 13, 12, V_BOTH, ("autoresets", "respawns")),
    Row("z1", lambda n: multi(n, niche_map(), 2, ["hamster"], 0, 2, weapons=["shotgun", "random"]), 37, 12, V_BOTH,
        ("autoresets", "respawns", "spawn_empty", "spawn_one", "spawn_short", "zombies_dropped")),
    Row("z64", _zlist(64), 13, 12, V_BOTH, ("autoresets", "respawns")),
    Row("z65", _zlist(65), 13, 12, V_BOTH, ("autoresets", "respawns")),
    Row("z512", _zlist(512), 7, 12, V_BOTH, ("autoresets", "respawns")),
    Row("z513", _zlist(513), 7, 12, V_BOTH + [V_LISTS_OFF], ("autoresets", "respawns")),
    Row("z600", _zlist(600), 7, 12, V_BOTH + [("leader_cand_hbm", {"fused": -1, "defer_respawn": -1,
                                                                   "lanes_per_env": 1}),
                                              ("leader_cand_lds", {"fused": -1, "defer_respawn": -1,
                                                                   "lanes_per_env": 16})],
        ("autoresets", "respawns")),
    # the spawn lists read from HBM by the reset and respawn work and by the tick (4 100 + nzs entries)
    Row("hbm0", _hbm(0), 5, 12, V_BOTH, ("autoresets", "respawns")),
    Row("hbm1", _hbm(1), 5, 12, V_BOTH, ("autoresets", "respawns", "spawn_short")),
    Row("hbm65", _hbm(65), 5, 12, V_BOTH, ("autoresets", "respawns")),
    Row("hbm512", _hbm(512), 5, 12, V_BOTH, ("autoresets", "respawns")),
    Row("hbm513", _hbm(513), 5, 12, V_BOTH + [V_LISTS_OFF], ("autoresets", "respawns")),
    Row("hbm600", _hbm(600), 5, 12, V_BOTH, ("autoresets", "respawns")),
    # player spawn lists
    Row("ps_exact", _pspawn(0), 13, 12, [V_FUSED, V_UNFUSED], ("autoresets", "spawn_exact")),
    Row("ps_plus1", _pspawn(1), 13, 12, [V_FUSED, V_UNFUSED], ("autoresets", "spawn_plus1")),
    # short of room
    Row("short", lambda n: multi(n, yard(12, 3), 2, ["hamster"], 0, 12, weapons=["shotgun", "random"], episode=3),
        13, 12, V_BOTH, ("autoresets", "respawns", "spawn_short", "zombies_dropped")),
    # more than 4 096 obstacles
    Row("walls4200", lambda n: multi(n, walls_map(), 2, [], 0, 4, weapons=["shotgun", "rifle"], episode=0), 5, 12,
        v_respawn(1)[:1] + v_respawn(-1), ("respawns",), setup="walls"),
]

# resets that fail: the players do not fit the player spawn list (ZS_ENOSPACE).  fail_agents: 3 bots take 3 of 4
# cells (n = k + 1), the 2 agents find 1 (n = 1: a shuffle without a draw); fail_agents0: the agent finds none;
# fail_bots: 4 bots over 3 cells
FAIL_ROWS = [
    Row("fail_agents", lambda n: multi(n, yard(4, 30), 2, bots(3), 3, 0), 5, 0, [V_FUSED, V_UNFUSED],
        ("player_fails", "spawn_one", "spawn_plus1")),
    Row("fail_agents0", lambda n: multi(n, yard(3, 30), 1, bots(3), 3, 0), 5, 0, [V_FUSED, V_UNFUSED],
        ("player_fails", "spawn_empty", "spawn_exact")),
    Row("fail_bots", lambda n: multi(n, yard(3, 30), 1, bots(4), 3, 0), 5, 0, [V_FUSED, V_UNFUSED],
        ("player_fails", "spawn_short")),
]


for _i, _r in enumerate(ROWS + FAIL_ROWS):
    _r.seed0 = 4000 + 100 * _i


def apply_walls_setup_oracle(o):
    for i in range(4096, N_WALLS):
        o.poke_obstacle_gone(i)


def oracle_run(row):
    """The oracle over the row's config, seeds, action stream and steps (next-step autoreset).  Returns
    (census summed over the envs, with "autoresets"; per env the (state, stream) after the last step; per env the
    trace [(obs, rewards, done, truncated, listed, reset)] of the steps; the reset observations; per env the state
    and stream after the first reset)."""
    from oracle.oracle import OracleEnv
    tot, envs, traces, obs0, after0 = {"autoresets": 0}, [], [], [], []
    for s in row.seeds():
        o = OracleEnv(row.make(1))
        o.seed(s)
        obs0.append(o.reset())
        after0.append((o.state(), o.get_rng()))
        if row.setup == "walls":
            apply_walls_setup_oracle(o)
        need, tr = False, []
        for t in range(1, row.steps + 1):
            if need:
                tr.append((o.reset(), None, False, False, np.ones(o.A, bool), True))
                need = False
                tot["autoresets"] += 1
            else:
                ob, r, d, tc, lb = o.step(row.actions([s], t, o.A)[0])
                tr.append((ob, r, d, tc, lb, False))
                need = d or tc
        for k, v in o.census().items():
            tot[k] = tot.get(k, 0) + v
        envs.append((o.state(), o.get_rng()))
        traces.append(tr)
    return tot, envs, traces, obs0, after0


def oracle_failing_reset(row):
    """Per seed: (zo_reset's return code, the stream record after it, the census, the state after it)."""
    from oracle.oracle import OracleEnv
    out = []
    for s in row.seeds():
        o = OracleEnv(row.make(1))
        o.seed(s)
        rc = o.reset_rc()
        out.append((rc, o.get_rng(), o.census(), o.state()))
    return out
