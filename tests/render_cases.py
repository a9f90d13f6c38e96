"""Shared by the render tests: the recorded fixtures (tests/golden/render_*.json.gz, make_render_golden.py), the frame a
recorded call's state composes to, the oracle-side body colours, and the table of the GPU rows (test_render.py).
"""
import base64
import hashlib
import json
import os
import zlib

import numpy as np

import golden_util as G
from libzombsole_amd import _abi
from libzombsole_amd import render as R

FIXTURES = ("render_field9x7_bot", "render_bridge_a4_bot", "render_safe_crowd_a2")


def recorded_atlas():
    with open(os.path.join(G.GOLDEN, "render_atlas.json"), encoding="utf-8") as f:
        return json.load(f)


def frame_hash(frame):
    return hashlib.sha256(np.ascontiguousarray(frame, dtype=np.uint8).tobytes()).hexdigest()[:16]


def unpack_frame(rr, W, H, palette):
    """A recorded full frame (one palette index per pixel, 255 black) as uint8 [10 H, 10 W, 3]."""
    idx = np.frombuffer(zlib.decompress(base64.b64decode(rr["frame"])), dtype=np.uint8).reshape(10 * H, 10 * W)
    pal = np.zeros((256, 3), dtype=np.uint8)
    pal[:len(palette)] = palette
    return pal[idx]


def fixture_colors(fx, builder):
    c = builder.cfg
    return R.slot_colors(builder.num_agents, list(c.bot_types[:c.num_bots]), max(c.initial_zombies, c.minimum_zombies))


def compose_recorded(fx, builder, rec, rr, atlas=None):
    """The frame of a recorded call from its canonical state (rec) and its recorded bodies (rr, the call's entry of
    the run's "render" list) alone."""
    m = builder.map
    W, H = m.size
    st = rec["state"]
    bots = list(builder.cfg.bot_types[:builder.cfg.num_bots])
    ents = []
    for kind, x, y, _life, _weapon, extra in st["dyn"]:
        col = R.BLUE if kind == _abi.THING_AGENT else R.GREEN if kind == _abi.THING_ZOMBIE else R.BOT_COLOR[int(bots[extra])]
        ents.append((x, y, col))
    gone = {i for i, _life, present in st["obst"] if not present}
    obst = [o for i, o in enumerate(m.obstacles) if i not in gone]
    bodies = {(x, y): c for x, y, c in rr["bodies"]}
    assert sorted(y * W + x for x, y in bodies) == st["dead"], "the recorded bodies are the state's dead cells"
    return R.compose(W, H, ents, obst, [(x, y, c) for (x, y), c in bodies.items()], m.objectives, atlas)


class BodyColors(object):
    """The expected body_col of one env, from the oracle's or the engine's death logs: the last death of a cell gives
    its colour; a reset clears it."""

    def __init__(self, W, H, colors):
        self.W, self.colors = W, colors
        self.row = np.zeros(W * H, dtype=np.uint8)
        self.seen = 0  # deaths applied since the object was made, whatever their colour

    def reset(self):
        self.row[:] = 0

    def deaths(self, log):
        for slot, _serial, x, y, _life in log:
            self.row[y * self.W + x] = self.colors[slot]
            self.seen += 1


# The GPU rows of test_render.py's kernel-against-compose test: name -> (config builder of n envs, steps).  Every map
# takes another path of k_render: 270-byte pixel rows (never 16-B aligned), aligned rows, strips without a left or an
# upper neighbour and with the clipped last column, a map with walls only, several bands per frame, more than 64 slots.
def _multi(map_name, agents, zombies, minimum, bots=(), rules="extermination", max_steps=9, **kw):
    def build(n, **over):
        opts = dict(kw, max_episode_steps=max_steps, render=True)
        opts.update(over)
        return _abi.multi_env_config(n, rules, list(bots), G.map_path(map_name) if isinstance(map_name, str) else map_name,
                                     [str(i) for i in range(agents)], initial_zombies=zombies, minimum_zombies=minimum, **opts)
    return build


def strip_map(w, h):
    """A w x h strip with no obstacles: players spawn at one end with the zombies next to them (deaths within a few
    steps), a zombie spawn cell and an objective at the far end, an objective on the first cell."""
    from libzombsole_amd.maps import Map
    cells = [(x, y) for y in range(h) for x in range(w)]
    return Map((w, h), [], cells[1:7], cells[7:18] + cells[-2:-1], [cells[0], cells[-1]], "strip%dx%d" % (w, h))


ROWS = {
    "field9x7": _multi("field9x7", 2, 6, 4, bots=("sniper", "hamster")),
    "safe8x5": _multi("safe_crowd", 2, 4, 4, bots=("randoman",), rules="safehouse"),
    "strip70x1": _multi(strip_map(70, 1), 2, 6, 6, bots=("terminator",)),
    "strip1x70": _multi(strip_map(1, 70), 2, 6, 6, bots=("terminator",)),
    "wall5x4": _multi("wall_hp", 2, 2, 2),
    "bridge64": _multi("bridge64", 2, 10, 8, bots=("terminator",), max_steps=0),
    "fort_e132": _multi("fort", 32, 100, 100, max_steps=0),
    # twelve zombies around two agents and four bots of four colours on the 9 x 7 field, no time limit: bodies of every
    # colour, later deaths on cells with a body, bodies on objectives; POKES opens cells for bodies on destroyed obstacles
    "crowd9x7": _multi("field9x7", 2, 12, 12, bots=("sniper", "hamster", "terminator", "randoman"), max_steps=0),
}
# [obstacle index, life] set before the first reset, in the oracle (poke_obstacle) and in the engine (set_state), as the
# wall_hp fixture does: the obstacle is in the world with life <= 0 at every reset (drawn) and the first tick removes it
POKES = {"crowd9x7": [[i, -5] for i in range(0, 40, 2)]}
STEPS = {"crowd9x7": 40, "fort_e132": 12}  # steps of a row (default 24)


# ---------------------------------------------------------------------------
# The oracle's side of a GPU row: the expected frame of every env after the reset and after every step, from the
# oracle's state and its death log alone (body colours accumulated here in Python), and the census of the case classes
# each env shows.  test_render_plan.py holds the census to REQUIRED; test_render.py compares the engine's frames.
# ---------------------------------------------------------------------------
SEED0 = 50  # env k of a row is seeded SEED0 + k
CLASSES = ("body_agent", "body_zombie", "body_bot", "recolour", "thing_on_body", "thing_on_objective", "body_on_objective",
           "body_on_gone_obstacle", "adj_h", "adj_v", "adj_d1", "adj_d2", "first_row", "last_row", "first_col", "last_col",
           "death_nonfinal4", "reset", "obstacle_life_le0")


def _state_parts(builder, st, row):
    m = builder.map
    W, _H = m.size
    bots = list(builder.cfg.bot_types[:builder.cfg.num_bots])
    ents = [(x, y, R.BLUE if kind == _abi.THING_AGENT else R.GREEN if kind == _abi.THING_ZOMBIE else R.BOT_COLOR[int(bots[extra])])
            for kind, x, y, _life, _weapon, extra in st["dyn"]]
    gone = {i for i, _life, present in st["obst"] if not present}
    obst = [o for i, o in enumerate(m.obstacles) if i not in gone]
    bodies = [(c % W, c // W, int(row[c])) for c in st["dead"]]
    return ents, obst, bodies, gone


import functools  # noqa: E402


@functools.lru_cache(maxsize=None)
def oracle_trace(row, n, steps, frames=True, every=1):
    """(expected, census): expected[t][k] the frame of env k after t steps (t = 0: the reset; None where frames is
    False or t is neither a multiple of `every` nor the last step), census[k] the set of CLASSES env k showed.
    Actions: the device policy's (actions.discrete_action_id)."""
    from libzombsole_amd import actions as A
    from oracle.oracle import OracleEnv
    builder = ROWS[row](1)
    m = builder.map
    W, H = m.size
    nA = builder.num_agents
    objectives = {tuple(o) for o in m.objectives}
    envs, rows, need, census = [], [], [False] * n, [set() for _ in range(n)]
    for k in range(n):
        o = OracleEnv(ROWS[row](1))
        o.seed(SEED0 + k)
        for i, life in POKES.get(row, []):
            if i < len(m.obstacles):
                o.poke_obstacle(i, life)
        o.reset()
        o.set_logs(True)
        envs.append(o)
        rows.append(np.zeros(W * H, dtype=np.uint8))
    bots = list(builder.cfg.bot_types[:builder.cfg.num_bots])
    seen_cells = [set() for _ in range(n)]  # cells with a body this episode

    def look(k, t):
        st = envs[k].state()
        ents, obst, bodies, gone = _state_parts(builder, st, rows[k])
        c = census[k]
        ecells = {(x, y) for x, y, _c in ents}
        bcells = {(x, y) for x, y, _c in bodies}
        gcells = {tuple(m.obstacles[i][:2]) for i in gone}
        drawn = ecells | bcells | objectives | {(o[0], o[1]) for o in obst}
        if any(present and life <= 0 for _i, life, present in st["obst"]):
            c.add("obstacle_life_le0")
        if ecells & bcells:
            c.add("thing_on_body")
        if ecells & objectives:
            c.add("thing_on_objective")
        if bcells & objectives:
            c.add("body_on_objective")
        if bcells & gcells:
            c.add("body_on_gone_obstacle")
        for x, y in drawn:
            for dx, dy, tag in ((1, 0, "adj_h"), (0, 1, "adj_v"), (1, 1, "adj_d1"), (-1, 1, "adj_d2")):
                if (x + dx, y + dy) in drawn:
                    c.add(tag)
            for hit, tag in ((y == 0, "first_row"), (y == H - 1, "last_row"), (x == 0, "first_col"), (x == W - 1, "last_col")):
                if hit:
                    c.add(tag)
        return R.compose(W, H, ents, obst, bodies, m.objectives) if frames and (t % every == 0 or t == steps) else None

    expected = [[look(k, 0) for k in range(n)]]
    for t in range(1, steps + 1):
        for k, o in enumerate(envs):
            if need[k]:
                o.reset()
                rows[k][:] = 0
                seen_cells[k].clear()
                need[k] = False
                census[k].add("reset")
                continue
            acts = np.stack([A.DISCRETE_TRIPLES[int(A.discrete_action_id(SEED0 + k, t, a, 7))] for a in range(nA)])
            _obs, _r, d, tr, _l = o.step(acts)
            need[k] = d or tr
            for kind, idx, x, y, _life, _before in o.death_log():
                col = R.BLUE if kind == _abi.THING_AGENT else R.GREEN if kind == _abi.THING_ZOMBIE else R.BOT_COLOR[int(bots[idx])]
                census[k].add("body_agent" if kind == _abi.THING_AGENT else "body_zombie" if kind == _abi.THING_ZOMBIE else
                              "body_bot" if col != R.BLUE else "body_bluebot")
                st_dead = rows[k][y * W + x]
                if (y * W + x) in seen_cells[k] and st_dead != col:
                    census[k].add("recolour")
                seen_cells[k].add(y * W + x)
                rows[k][y * W + x] = col
                if t % 4:
                    census[k].add("death_nonfinal4")
        expected.append([look(k, t) for k in range(n)])
    return expected, census


_ALL = frozenset(CLASSES)
_ADJ = frozenset(("adj_h", "adj_v", "adj_d1", "adj_d2"))
_EDGES = frozenset(("first_row", "last_row", "first_col", "last_col"))
# The classes every row must show in three envs or more of its first 13, by the oracle alone (test_render_plan.py).
REQUIRED = {
    "field9x7": _ADJ | _EDGES | {"body_agent", "body_zombie", "thing_on_body", "thing_on_objective", "death_nonfinal4", "reset"},
    "safe8x5": _ADJ | _EDGES | {"body_agent", "body_zombie", "body_on_objective", "thing_on_body", "thing_on_objective", "reset"},
    "strip70x1": _EDGES | {"adj_h", "body_zombie", "thing_on_body", "thing_on_objective", "reset"},
    "strip1x70": _EDGES | {"adj_v", "body_zombie", "thing_on_body", "thing_on_objective", "reset"},
    "wall5x4": _ADJ | _EDGES | {"body_zombie", "thing_on_body", "reset"},
    "bridge64": _ADJ | _EDGES | {"body_zombie", "thing_on_body", "death_nonfinal4"},
    "fort_e132": _ADJ | _EDGES | {"body_zombie", "thing_on_body", "death_nonfinal4"},
    "crowd9x7": _ALL,
}


def steps_of(row):
    return STEPS.get(row, 24)
