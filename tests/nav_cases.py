"""Shared by the path-distance tests: the case table (one row = a config the oracle and the engine both run), the
oracle-side trace of a row with its census, the independent cell-by-cell BFS the model is held to, and the text form
tests/nav_host.cpp reads.  Each row is the smallest shape at which a piece of the search can go wrong.
"""
import collections
import functools

import numpy as np

import entity_obs_cases as EC
import golden_util as G
import render_cases as RC
from libzombsole_amd import _abi
from libzombsole_amd import nav as NV
from libzombsole_amd.entity_obs import Static
from libzombsole_amd.maps import Map

SEED0 = 50
CLASSES = ("unreachable", "unreachable_neighbour", "tie", "cut", "on_source", "absent_agent", "obstacle_removed")


def open_map(w, h):
    """A w x h field without obstacles: an objective on the first cell, the zombie spawns next to it, the players at the
    far end (the objective field crosses every word of a row; the two fields' sources lie at opposite ends)."""
    cells = [(x, y) for y in range(h) for x in range(w)]
    n = len(cells)
    if n == 1:
        return Map((w, h), [], cells, [], cells, "open1x1")
    k = max(1, min(8, n // 3))
    return Map((w, h), [], cells[-k:], cells[1:1 + k], [cells[0]], "open%dx%d" % (w, h))


GOLDEN_MAPS = ("nav_serpentine", "nav_pocket_in", "nav_pocket_out", "wall_hp")  # tests/golden/maps/<name>.txt


def _multi(map_, agents, zombies, minimum, bots=(), max_steps=0, **kw):
    def build(n, **over):
        opts = dict(kw, max_episode_steps=max_steps)
        opts.update(over)
        mp = G.map_path(map_) if map_ in GOLDEN_MAPS else map_
        return _abi.multi_env_config(n, "extermination", list(bots), mp, [str(i) for i in range(agents)],
                                     initial_zombies=zombies, minimum_zombies=minimum, **opts)
    return build


# name -> (builder of n envs, steps, caps beside 32766, pokes [[obstacle, life]] applied before the first reset)
ROWS = {
    "open31x3": (_multi(open_map(31, 3), 2, 3, 3), 8, (), ()),
    "open32x3": (_multi(open_map(32, 3), 2, 3, 3), 8, (), ()),
    "open33x3": (_multi(open_map(33, 3), 2, 3, 3), 8, (1,), ()),
    "open65x2": (_multi(open_map(65, 2), 2, 3, 3), 8, (), ()),  # a third word per row
    "strip70x1": (_multi(RC.strip_map(70, 1), 2, 6, 6, bots=("terminator",)), 8, (16,), ()),  # H = 1
    "open2x65": (_multi(open_map(2, 65), 2, 3, 3), 8, (), ()),  # 65 words: one past the lanes' first pass
    "open1x1": (_multi(open_map(1, 1), 1, 0, 0), 3, (), ()),
    "serpentine": (_multi("nav_serpentine", 2, 4, 4), 12, (1, 80), ()),  # 168 moves end to end on a 33 x 9 map
    "pocket_in": (_multi("nav_pocket_in", 2, 2, 2), 8, (), ()),  # agents and zombies sealed in, objectives outside
    "pocket_out": (_multi("nav_pocket_out", 2, 2, 2), 8, (), ()),  # agents and objectives sealed in, zombies outside
    "arduino": (_multi("arduino", 2, 6, 6, bots=("sniper",)), 8, (), ()),  # no objectives
    "easy_exit": (_multi("easy_exit", 2, 4, 4), 8, (), ()),  # 32 objective cells around the players' spawns
    "crowd9x7": (RC.ROWS["crowd9x7"], 16, (3,), tuple(map(tuple, RC.POKES["crowd9x7"]))),  # agents die; obstacles fall
    "wall5x4": (_multi("wall_hp", 2, 1, 1), 4, (), ((6, -5), (2, -5))),  # a wall of the sealed room falls at the first tick
    "bridge_a4": (lambda n, **over: EC.builder("bridge_a4", n, **over), 8, (40,), ()),  # 28 objectives, A = 4 and bots
    "fort_e132": (RC.ROWS["fort_e132"], 4, (), ()),  # E > 64, A = 32
}
CAP = NV.MAX_DIST


def builder(row, n, **over):
    if row in ("crowd9x7", "fort_e132"):  # render_cases' builders: without their render flag
        over.setdefault("render", False)
    return ROWS[row][0](n, **over)


def steps_of(row):
    return ROWS[row][1]


def caps_of(row):
    return (CAP,) + tuple(ROWS[row][2])


def pokes_of(row):
    return ROWS[row][3]


# ---------------------------------------------------------------------------
# the independent statement: a deque over cells, no code shared with libzombsole_amd/nav.py
# ---------------------------------------------------------------------------
def naive_field(view, static, which, max_dist):
    W, H = static.W, static.H
    blocked = {static.obstacles[i] for i in range(len(static.obstacles)) if int(view.obst_present[i])}
    if which == 1:
        src = list(static.objectives)
    else:
        src = [(int(e[2]), int(e[3])) for s, e in enumerate(view.ent) if s >= view.A + view.P and int(e[1])]
    dist = {}
    todo = collections.deque()
    for c in src:
        if 0 <= c[0] < W and 0 <= c[1] < H and c not in blocked and c not in dist:
            dist[c] = 0
            todo.append(c)
    while todo:
        x, y = todo.popleft()
        if dist[(x, y)] == max_dist:
            continue
        for c in ((x, y + 1), (x - 1, y), (x, y - 1), (x + 1, y)):
            if 0 <= c[0] < W and 0 <= c[1] < H and c not in blocked and c not in dist:
                dist[c] = dist[(x, y)] + 1
                todo.append(c)
    out = np.full((H, W), 0xFFFF, dtype=np.uint16)
    for (x, y), v in dist.items():
        out[y, x] = v
    return out


def naive_rows(view, static, fields, max_dist):
    bits = [b for b in (1, 2) if fields & b]
    out = np.zeros((view.A, len(bits), 8), dtype=np.int16)
    for f, b in enumerate(bits):
        d = naive_field(view, static, b, max_dist)
        for a in range(view.A):
            if not int(view.ent[a][1]):
                continue
            x, y = int(view.ent[a][2]), int(view.ent[a][3])
            w = []
            for cx, cy in ((x, y), (x, y + 1), (x - 1, y), (x, y - 1), (x + 1, y)):
                inside = 0 <= cx < static.W and 0 <= cy < static.H
                w.append(int(d[cy, cx]) if inside and d[cy, cx] != 0xFFFF else -1)
            nb = w[1:]
            lo = hi = -1
            for k in range(4):
                if nb[k] >= 0 and (lo < 0 or nb[k] < nb[lo]):
                    lo = k
                if nb[k] >= 0 and (hi < 0 or nb[k] > nb[hi]):
                    hi = k
            out[a, f] = w + [lo, hi, 1 | (2 if w[0] == 0 else 0)]
    return out


def classes_of(view, static, cap):
    """The census classes the env's state shows (fields = both), by the naive BFS alone; cap: the row's smallest cap."""
    c = set()
    rows = naive_rows(view, static, 3, CAP)
    cut = naive_rows(view, static, 3, cap) if cap != CAP else rows
    for a in range(view.A):
        if not int(view.ent[a][1]):
            c.add("absent_agent")
            continue
        for f in range(2):
            r = [int(v) for v in rows[a, f]]
            nb = [v for v in r[1:5] if v >= 0]
            if r[0] < 0:
                c.add("unreachable")
            elif len(nb) < 4:
                c.add("unreachable_neighbour")
            if nb and (nb.count(min(nb)) > 1 or nb.count(max(nb)) > 1) and min(nb) != max(nb):
                c.add("tie")
            if r[0] == 0:
                c.add("on_source")
            if any(int(cut[a, f, k]) < 0 <= r[k] for k in range(5)):
                c.add("cut")
    if (np.asarray(view.obst_present) == 0).any():
        full = EC.View(view.A, view.P, [list(e) for e in view.ent], np.ones(len(view.obst_present), dtype=np.int64))
        if any(not np.array_equal(naive_field(view, static, b, CAP), naive_field(full, static, b, CAP)) for b in (1, 2)):
            c.add("obstacle_removed")
    return c


@functools.lru_cache(maxsize=None)
def oracle_trace(row, n=13):
    """(views, states, census): views[t][k] the oracle's state of env k after t steps as an entity_obs_cases.View
    (t = 0: the reset; the autoreset in the step after an env ended), states[t][k] the same as the oracle's dict,
    census[k] the classes env k showed.  Actions: the device policy's."""
    from libzombsole_amd import actions as A
    from oracle.oracle import OracleEnv
    b = builder(row, 1)
    static = Static.of_map(b.map)
    nA = b.num_agents
    cap = min(caps_of(row))
    envs, need, census = [], [False] * n, [set() for _ in range(n)]
    for k in range(n):
        o = OracleEnv(builder(row, 1))
        o.seed(SEED0 + k)
        for i, life in pokes_of(row):
            if i < len(b.map.obstacles):
                o.poke_obstacle(i, life)
        o.reset()
        envs.append(o)

    def look(k):
        st = envs[k].state()
        v = EC.oracle_view(b, st)
        census[k] |= classes_of(v, static, cap)
        return v, st

    both = [[look(k) for k in range(n)]]
    for t in range(1, steps_of(row) + 1):
        for k, o in enumerate(envs):
            if need[k]:
                o.reset()
                need[k] = False
                continue
            acts = np.stack([A.DISCRETE_TRIPLES[int(A.discrete_action_id(SEED0 + k, t, a, 7))] for a in range(nA)])
            _obs, _r, d, tr, _l = o.step(acts)
            need[k] = d or tr
        both.append([look(k) for k in range(n)])
    return [[v for v, _ in r] for r in both], [[s for _, s in r] for r in both], census


def census_counts(n=13):
    """class -> the number of envs, across the table, that show it."""
    tot = collections.Counter()
    for row in ROWS:
        for s in oracle_trace(row, n)[2]:
            tot.update(s)
    return tot


def host_text(cases):
    """[(view, static, fields, max_dist)] as the text nav_host reads."""
    lines = [str(len(cases))]
    for v, st, fields, cap in cases:
        lines.append("%d %d %d %d %d %d %d %d %d" % (st.W, st.H, v.A, v.P, len(v.ent), len(st.obstacles), len(st.objectives),
                                                     fields, cap))
        lines += ["%d %d %d" % tuple(int(x) for x in e[1:4]) for e in v.ent]
        lines += ["%d %d %d" % (x, y, int(v.obst_present[i])) for i, (x, y) in enumerate(st.obstacles)]
        lines += ["%d %d" % o for o in st.objectives]
    return "\n".join(lines) + "\n"
