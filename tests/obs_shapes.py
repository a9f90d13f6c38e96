"""The shapes of the general observation encoder (csrc/zs_obs.hpp: k_obs, and the same obs_build / obs_stream run by
the step launch when the plan sets fobs), one row per shape, and the simple encoding in the store-stream kernels.
obs_instantiations.py's rows are all the registered shape (surroundings of width 21, channels, 1, 2 or 4
observations per env); everything else a config can ask for is here: the scope, the encoding, the window width
and the tier of the LDS image that obs_plan() (csrc/zs_obs_plan.hpp) falls back to by size.

Every row states what the plan must resolve it to, (kernel, masked kernel, window map, staged HP, static tables,
k_obs waves per workgroup, fobs), and the function of obs_stream() that therefore encodes it:

  fast21    obs_stream_fast<T, 21>: static tables, staged HP, window map, surroundings of width 21
  fast0     obs_stream_fast<T, 0>:  the same at any other width and in the world scope
  gen_win   obs_stream_gen with the window map and staged HP (no static tables: the map's obstacles are not in
            row-major order)
  gen_hbm   obs_stream_gen with the window map, HP read from HBM (the image with HP is past 32 KiB)
  gen_scan  obs_stream_gen with the per-cell entity scan (the window map alone is past 32 KiB)
  pipe / gather   k_obs_pipe / k_obs_gather (their own cell walk), here under the simple encoding

The claims were written from obs_plan() and the boundaries found with the compiled plan on the CPU;
test_obs_shapes_plan.py holds every row to the compiled plan, test_obs_shapes.py runs every row on the GPU.

Row stepping.  obs_stream_fast<T, 0> and obs_stream_gen walk cells lane, lane + 64, ... with step_r = 64 / ww,
step_q = 64 - step_r * ww and one wrap: ww = 3 (21, 1), 5 (12, 4), 19 (3, 7), 23 (2, 18), 63 (1, 1), 64 (1, 0),
65 (0, 64), 127 and 130 (0, 64), and ww = 1 and 2 (64, 0 and 32, 0), which only the world scope has.

Tier boundaries (win = align16(observations x w x w) beside 12 B an entity, the dead-body, present and HP words):
on the 9 x 7 field one observation keeps the window map up to w = 179 (32 041 -> 32 048 B, image 32 288 B) and
loses it at 181 (the image is then 112 B, and the step launch takes it); four agents keep it up to 89 and lose it at
91; one city128 observation stages HP up to w = 123 (image 32 464 B) and reads it from HBM from 125 on (3 689
obstacles: 14 756 B); on the 9 x 7 field k_obs runs four waves a workgroup up to w = 127 (image 16 288 B) and one from
129 on, and the step launch writes the observations itself up to w = 127 too (image + 32 B of tables <= 16 KiB).
"""
import numpy as np

from libzombsole_amd import _abi
from libzombsole_amd import actions as A
from libzombsole_amd.maps import Map

import geometry_shapes
import obs_instantiations as I

EPISODE = 5
DT = {"i16": _abi.DTYPE_I16, "i32": _abi.DTYPE_I32, "i64": _abi.DTYPE_I64}
DTS = ("i64", "i32", "i16")
ENCS = ("simple", "channels")
FUNCS = ("fast21", "fast0", "gen_win", "gen_hbm", "gen_scan")


# -- maps ------------------------------------------------------------------------------------------------------------
def field(W, H, reverse=False):
    """A generated W x H field, cells numbered row-major: walls at every 11th cell (from 3), boxes at every 13th
    (from 5), objectives at every 17th (from 7); the free cells at multiples of 5 (cell 0 among them) are the
    player spawns, those one before and the last cell of the map the zombie spawns.  reverse: the obstacles listed
    last cell first, so that the map is not in rank order and the plan stages no static tables."""
    obst, objs, ps, zs = [], [], [], []
    for c in range(W * H):
        xy = (c % W, c // W)
        if c == W * H - 1 or c % 5 == 4:
            zs.append(xy)
        elif c % 5 == 0:
            ps.append(xy)
        elif c % 11 == 3:
            obst.append(xy + (_abi.THING_WALL,))
        elif c % 13 == 5:
            obst.append(xy + (_abi.THING_BOX,))
        elif c % 17 == 7:
            objs.append(xy)
    if reverse:
        obst.reverse()
    return Map((W, H), obst, ps, zs, objs, name="field%dx%d%s" % (W, H, "r" if reverse else ""))


WORLD_SIZES = ((1, 70), (70, 1), (2, 33), (3, 50), (63, 5), (64, 5), (65, 5), (130, 3))
MAPS = {"small": lambda: field(9, 7), "small_rev": lambda: field(9, 7, reverse=True), "bridge64": lambda: "bridge64",
        "city128": lambda: "city128", "geo183x182": lambda: geometry_shapes.closest_map(183, 182)}
for _w, _h in WORLD_SIZES:
    MAPS["field%dx%d" % (_w, _h)] = (lambda w=_w, h=_h: field(w, h))


def map_text(m):
    """The map as a map file's text ('w' wall, 'b' box, 'o' objective, 'p' / 'z' spawn cells, '.' free)."""
    W, H = m.size
    rows = [["."] * W for _ in range(H)]
    cells = [((x, y), "w" if k == _abi.THING_WALL else "b") for x, y, k in m.obstacles]
    cells += [(c, "o") for c in m.objectives] + [(c, "p") for c in m.player_spawns] + [(c, "z") for c in m.zombie_spawns]
    for (x, y), ch in cells:
        assert rows[y][x] == ".", (x, y)
        rows[y][x] = ch
    return "".join("".join(r) + "\n" for r in rows)


# the maps of the reference fixtures obs_* (tests/golden/make_golden.py), by the map name their kwargs hold; the file is
# written to a temporary directory when a fixture is recorded or replayed (golden_util.map_path)
FIXTURE_MAPS = {"field9x7": lambda: field(9, 7), "field63x5": lambda: field(63, 5)}


def single(map_name, scope, enc, dt, zombies=6, bots=("sniper",)):
    """The single surface: one agent's window, or the world."""
    return lambda n: _abi.single_env_config(n, "extermination", list(bots), MAPS[map_name](), "0", initial_zombies=zombies,
                                            minimum_zombies=2, observation_scope=scope,
                                            observation_position_encoding=enc, obs_dtype=DT[dt],
                                            max_episode_steps=EPISODE)


def multi(map_name, agents, w, enc, dt, zombies=6):
    """The multi surface: one block per agent (under the simple encoding too: the engine's extension)."""
    return lambda n: _abi.multi_env_config(n, "extermination", [], MAPS[map_name](), [str(a) for a in range(agents)],
                                           initial_zombies=zombies, minimum_zombies=2,
                                           observation_surroundings_width=w,
                                           observation_position_encoding_style=enc, obs_dtype=DT[dt],
                                           max_episode_steps=EPISODE)


def stream_map(map_name, nobs, enc, dt):
    """obs_instantiations.py's two configs under an encoding of choice."""
    def make(n):
        b = I.MAPS[map_name](n, DT[dt], nobs)
        b.cfg.obs_encoding = _abi.parse_encoding(enc)
        return b
    return make


def actions(seeds, t, n_agents):
    """zs_gen_actions' discrete stream at step t: int32 [len(seeds)][n_agents][3]."""
    return np.array([[A.DISCRETE_TRIPLES[A.discrete_action_id(s, t, a, 7)] for a in range(n_agents)] for s in seeds],
                    dtype=np.int32)


# -- pokes -----------------------------------------------------------------------------------------------------------
def view_rect(builder, state, a=0):
    """(x0, y0, x1, y1), inclusive: the map cells observation a shows."""
    W, H = builder.map.size
    if builder.cfg.obs_scope == _abi.OBS_WORLD:
        return 0, 0, W - 1, H - 1
    half = builder.cfg.obs_width // 2
    ax, ay = state["agents"][a][:2]
    return max(ax - half, 0), max(ay - half, 0), min(ax + half, W - 1), min(ay + half, H - 1)


def poke_plan(builder, state, rng, e):
    """What the tests poke into env e after its trajectory, from the oracle's canonical state alone: (dead-body
    cells, {obstacle: life}, the obstacles taken out of the world).  Random bodies and a dozen random obstacle lives
    (the non-positive ones cleaned up at a coin's toss), obstacle 0 just below the int16 range, and, on the three
    obstacles nearest to agent 0 inside its observation: the nearest damaged, still in the world, with a body under
    it (the obstacle shows); the second cleaned up with a body on its cell (the body shows); the third at life
    -40 000 (int16 saturates it)."""
    W, H = builder.map.size
    obst = builder.map.obstacles
    O, cells = len(obst), W * H
    dead = [int(c) for c in rng.choice(cells, size=min(cells // 2, (3, 40, 300)[e % 3]), replace=False)]
    lives, gone = {}, set()
    for i in rng.choice(O, size=min(O, 12), replace=False):
        lives[int(i)] = int(rng.integers(-32000, 199))
        if lives[int(i)] <= 0 and rng.integers(2):
            gone.add(int(i))
    lives[0] = -32769
    gone.discard(0)
    x0, y0, x1, y1 = view_rect(builder, state)
    ax, ay = state["agents"][0][:2]
    absent = {i for i, _, present in state["obst"] if not present}
    near = sorted((i for i in range(1, O) if i not in absent and x0 <= obst[i][0] <= x1 and y0 <= obst[i][1] <= y1),
                  key=lambda i: ((obst[i][0] - ax) ** 2 + (obst[i][1] - ay) ** 2, i))
    for k, i in enumerate(near[:3]):
        gone.discard(i)
        lives[i] = (1 + e % 9, -5 - e, -40000)[k]
        if k == 1:
            gone.add(i)
        if k < 2:
            dead.append(obst[i][1] * W + obst[i][0])
    return sorted(set(dead)), lives, sorted(gone)


def poke_oracle(o, plan, W):
    dead, lives, gone = plan
    for c in dead:
        o.poke_dead(c % W, c // W)
    for i, life in lives.items():
        o.poke_obstacle(i, life)
    for i in gone:
        o.poke_obstacle_gone(i)


def poke_engine(eng, e, plan):
    dead, lives, gone = plan
    st = eng.get_state(e)
    dw = st.dead_words.view(np.uint32)  # writes through to the record
    for c in dead:
        dw[c >> 5] |= np.uint32(1 << (c & 31))
    for i, life in lives.items():
        st.obst_life[i] = life
    for i in gone:
        st.obst_present[i] = 0
    eng.set_state(e, st)


# -- rows ------------------------------------------------------------------------------------------------------------
class Row(object):
    """plan: (obs_kernel as describe() names it, obs_kernel_masked, window map, staged HP, static tables, k_obs waves
    per workgroup, fobs).  func: the function that encodes the row's unmasked launches."""

    def __init__(self, rid, make, plan, func, dt, enc, n=13, steps=12, launch=None, lanes=0, step_kernel=None):
        self.id, self.make, self.plan, self.func, self.dt, self.enc = rid, make, plan, func, dt, enc
        self.n, self.steps, self.launch, self.lanes, self.step_kernel = n, steps, dict(launch or {}), lanes, step_kernel
        self.seed0 = None

    def builder(self, n=None):
        b = self.make(self.n if n is None else n)
        b.cfg.lanes_per_env = self.lanes
        return b.set_launch(self.launch)

    def agent_ids(self):
        """Every row's agents are created with the ids "0", "1", ... in order."""
        return list(range(self.builder(1).num_agents))

    def seeds(self, n=None):
        return [self.seed0 + 13 * i for i in range(self.n if n is None else n)]


STEP = "step launch"
ROWS = []
_k = {}


def _next(seq):
    """The members of seq in turn, each sequence on its own count."""
    _k[seq] = _k.get(seq, -1) + 1
    return seq[_k[seq] % len(seq)]


def _add(*a, **kw):
    ROWS.append(Row(*a, **kw))


# row stepping, surroundings, single surface.  On the 9 x 7 field the step launch writes the observations itself (fobs)
# and every window from 19 on hangs over the padding on all four sides; bridge64 has more than 64 zombie spawn cells,
# so its zombies respawn in k_respawn after the tick and k_obs encodes every step (one wave a workgroup at w = 127).
SURR_WIDTHS = (3, 5, 19, 23, 63, 65, 127)
for _m in ("small", "bridge64"):
    for _w in SURR_WIDTHS:
        for _enc in ENCS:
            _dt = _next(DTS)
            _plan = (STEP, "k_obs", True, True, True, 4, 1) if _m == "small" else \
                ("k_obs", "k_obs", True, True, True, 4 if _w < 127 else 1, 0)
            _add("surr%d-%s-%s-%s" % (_w, _m, _enc, _dt), single(_m, "surroundings:%d" % _w, _enc, _dt), _plan, "fast0",
                 _dt, _enc, n=_next((13, 37)))
# row stepping, world scope: the step launch up to 64 zombie spawn cells (64 x 5), k_obs past them
for _name in ["field%dx%d" % s for s in WORLD_SIZES] + ["bridge64"]:
    for _enc in ENCS:
        _dt = _next(DTS)
        _plan = ("k_obs", "k_obs", True, True, True, 4, 0) if _name in ("field65x5", "field130x3", "bridge64") else \
            (STEP, "k_obs", True, True, True, 4, 1)
        _add("world-%s-%s-%s" % (_name, _enc, _dt), single(_name, "world", _enc, _dt), _plan, "fast0", _dt, _enc,
             n=_next((13, 37)))
# no static tables (obstacles out of rank order): obs_stream_gen with the window map and staged HP
for _dt in DTS:
    for _enc in ENCS:
        _scope = _next(("surroundings:5", "world", "surroundings:23"))
        _add("norank-%s-%s-%s" % (_scope.replace(":", ""), _enc, _dt), single("small_rev", _scope, _enc, _dt),
             (STEP, "k_obs", True, True, False, 4, 1), "gen_win", _dt, _enc)
# tiers by size.  The window map: 179 | 181 (one observation), 89 | 91 (four agents)
for _dt in DTS:
    for _enc in ENCS:
        _add("scan181-%s-%s" % (_enc, _dt), single("small", "surroundings:181", _enc, _dt),
             (STEP, "k_obs", False, False, True, 4, 1), "gen_scan", _dt, _enc, steps=6)
_add("win179-simple-i16", single("small", "surroundings:179", "simple", "i16"), ("k_obs", "k_obs", True, True, True, 1, 0),
     "fast0", "i16", "simple", steps=6)
_add("win179-channels-i64", single("small", "surroundings:179", "channels", "i64"), ("k_obs", "k_obs", True, True, True, 1, 0),
     "fast0", "i64", "channels", steps=6)
_add("a4win89-channels-i32", multi("small", 4, 89, "channels", "i32"), ("k_obs", "k_obs", True, True, True, 1, 0), "fast0",
     "i32", "channels", steps=6)
_add("a4scan91-simple-i32", multi("small", 4, 91, "simple", "i32"), (STEP, "k_obs", False, False, True, 4, 1), "gen_scan",
     "i32", "simple", steps=6)
# staged HP: city128's 3 689 obstacles beside one window of 123 | 125
for _dt in DTS:
    for _enc in ENCS:
        _add("hbm125-%s-%s" % (_enc, _dt), single("city128", "surroundings:125", _enc, _dt, zombies=20),
             ("k_obs", "k_obs", True, False, True, 1, 0), "gen_hbm", _dt, _enc, steps=6)
_add("hp123-simple-i64", single("city128", "surroundings:123", "simple", "i64", zombies=20),
     ("k_obs", "k_obs", True, True, True, 1, 0), "fast0", "i64", "simple", steps=6)
# waves per workgroup 4 | 1 and the step launch's 16 KiB, both between 127 (the surr127-small rows) and 129
_add("wpg129-simple-i32", single("small", "surroundings:129", "simple", "i32"), ("k_obs", "k_obs", True, True, True, 1, 0),
     "fast0", "i32", "simple", steps=6)
_add("wpg129-channels-i16", single("small", "surroundings:129", "channels", "i16"), ("k_obs", "k_obs", True, True, True, 1, 0),
     "fast0", "i16", "channels", steps=6)
# a map of more than 32 768 cells has no static tables either (DW > 1024)
_add("bigmap-surr5-simple-i64", single("geo183x182", "surroundings:5", "simple", "i64", zombies=2, bots=()),
     (STEP, "k_obs", True, True, False, 4, 1), "gen_win", "i64", "simple", steps=6)
# width 21 with 3 and 5 agents: no store-stream kernel takes the count, k_obs encodes full and masked launches
for _dt in DTS:
    for _enc in ENCS:
        _a = _next((3, 5))
        _add("w21a%d-%s-%s" % (_a, _enc, _dt), multi("bridge64", _a, 21, _enc, _dt, zombies=12),
             ("k_obs", "k_obs", True, True, True, 4, 0), "fast21", _dt, _enc, n=_next((13, 37)), launch={"fobs": -1})
SHAPE_ROWS = list(ROWS)

# the simple encoding in the store-stream kernels: obs_instantiations.py's overrides, maps alternating; 24 steps, for
# bridge64's episodes there are 12 steps long
STREAM_ROWS = []
for _v in ("pipe", "gather"):
    for _dt in DTS:
        for _nobs in (1, 2, 4):
            _m = ("bridge64", "wall_hp")[len(STREAM_ROWS) % 2]
            _lo, _kern, _masked = I.VARIANTS[_v][:3]
            STREAM_ROWS.append(Row("%s-simple-%s-x%d-%s" % (_v, _dt, _nobs, _m), stream_map(_m, _nobs, "simple", _dt),
                                   (_kern, _masked, True, _v == "pipe", True, 4, 0), _v, _dt, "simple",
                                   n=_next((13, 37, 67)), launch=_lo, steps=24))
# the staged kernels stay off the simple encoding whatever the overrides ask for
for _v, _kern, _masked, _func in (("patch", "k_obs_pipe", "k_obs", "pipe"), ("ring_patched", "k_obs_pipe", "k_obs", "pipe"),
                                  ("pbring", "k_obs_gather", "k_obs_gather", "gather")):
    STREAM_ROWS.append(Row("%s_asked-simple-i16-x2-bridge64" % _v, stream_map("bridge64", 2, "simple", "i16"),
                           (_kern, _masked, True, _func == "pipe", True, 4, 0), _func, "i16", "simple", n=37,
                           launch=I.VARIANTS[_v][0], steps=24))
ROWS += STREAM_ROWS

# where it is encoded: three small rows, each by k_obs alone, by the step launch's tick workgroups at 1, 8 and 64
# lanes an env, by its reset work (fused) and by the unfused launches
WHERE = {"surr7-channels": lambda dt: multi("small", 2, 7, "channels", dt),
         "surr5-simple": lambda dt: single("small", "surroundings:5", "simple", dt),
         "world-simple": lambda dt: single("field63x5", "world", "simple", dt)}
WHERE_VARIANTS = (("k_obs", {"fobs": -1}, 0, "k_obs", 0), ("tickG1", {"fobs": 1}, 1, STEP, 1), ("tickG8", {"fobs": 1}, 8, STEP, 1),
                  ("tickG64", {"fobs": 1}, 64, STEP, 1), ("fused", {"fobs": 1, "fused": 1}, 0, STEP, 1),
                  ("unfused", {"fobs": 1, "fused": -1}, 0, STEP, 1))
WHERE_ROWS = []
for _name, _mk in WHERE.items():
    for _vn, _lo, _g, _kern, _fobs in WHERE_VARIANTS:
        _dt = _next(DTS)
        WHERE_ROWS.append(Row("where-%s-%s-%s" % (_name, _vn, _dt), _mk(_dt), (_kern, "k_obs", True, True, True, 4, _fobs), "fast0",
                              _dt, _name.split("-")[1], n=37, launch=_lo, lanes=_g,
                              step_kernel={"fused": "k_step", "unfused": "k_tick"}.get(_vn)))
ROWS += WHERE_ROWS

# first seeds: 83000 + 100 * the row's place, plus the first multiple of 7 at which the oracle's run of the row shows
# what test_obs_shapes_plan.py asks of it (searched with the oracle alone)
_SEED_SHIFT = {"world-field1x70-simple-i32": 7}
for _i, _r in enumerate(ROWS):
    _r.seed0 = 83000 + 100 * _i + _SEED_SHIFT.get(_r.id, 0)
BY_ID = {r.id: r for r in ROWS}
assert len(BY_ID) == len(ROWS)

# -- what a row's run must show ------------------------------------------------------------------------------------
EDGES = ("top", "bottom", "left", "right")
POKED = ("body_under_obstacle", "damaged", "cleaned_up")


def required(row):
    """The content classes of test_obs_shapes_plan.census() that the oracle's run of the row must show in three envs
    or more.  The rule, by what a map and a window can show in episodes of five steps:

      * the generated fields (players spawn from the first cell on, zombies up to the last): a thing on all four
        edges of what an observation shows of the map; for windows, an off-map cell on all four sides; the three
        poked classes, except `cleaned_up` at w = 3 (the pokes clean up the second-nearest obstacle in view, and nine
        cells seldom hold two);
      * bridge64 (agents spawn on its right-hand side, zombies far from them): a thing in the first and the last row
        of a window of 21; off-map cells above, below and to the right from w = 63, to the left too at 127; the
        poked classes from w = 19 and in the world scope (no obstacle stands within two cells of a spawn cell);
      * the wall map (5 x 4, no zombies): off-map cells on all four sides, the poked classes;
      * city128 at w = 125 (agents spawn towards its lower right): off-map cells below and to the right, the poked
        classes; the 183 x 182 map at w = 5 (players in its first corner): above and to the left, the poked classes;
      * every multi row: a second living agent inside the first one's window."""
    b = row.builder(1)
    world = b.cfg.obs_scope == _abi.OBS_WORLD
    w = b.cfg.obs_width
    name = b.map.name or ""
    need = []
    if name.startswith("field"):
        need += EDGES + (() if world else tuple("off_" + e for e in EDGES))
        need += POKED if world or w > 3 else POKED[:2]
    elif name.startswith("bridge64"):
        if not world and w == 21:
            need += ["top", "bottom"]
        if not world and w >= 63:
            need += ["off_top", "off_bottom", "off_right"] + (["off_left"] if w >= 127 else [])
        if world or w >= 19:
            need += POKED
    elif name.startswith("wall_hp"):
        need += ["off_" + e for e in EDGES] + list(POKED)
    elif name.startswith("city128"):
        need += ["off_bottom", "off_right"] + list(POKED)
    elif name.startswith("geo183x182"):
        need += ["off_top", "off_left"] + list(POKED)
    else:
        raise AssertionError("no census rule for map %r" % name)
    if not world and b.obs_shape()[0] > 1:
        need.append("second")
    return list(need)


# what zs_create refuses: no image tier of a 1 040 x 1 040 world fits 64 KiB (the dead-body row alone is 135 KB)
REFUSED = geometry_shapes.REFUSED["world_obs"]

# -- life edges under the simple encoding ------------------------------------------------------------------------------
# obstacle lives round every point where 15 * min(life, 100) // 100 changes its form: the cap at 100, the floor
# division's sign change (7 | 6 -> 1 | 0, -1, -6 | -7 -> -1 | -2), the int16 floor of the life itself, the encoder's
# 32-bit fast path down to -(1 << 26) and the 64-bit one below, and the lowest life the engine holds
OBSTACLE_LIVES = (199, 100, 7, 6, 1, 0, -1, -6, -7, -100, -32768, -32769, -(1 << 26), -(1 << 26) - 1, -2147483647)
ENTITY_LIFE = 137  # above the cap of 100: 256 * code + 16 * weapon + 15
