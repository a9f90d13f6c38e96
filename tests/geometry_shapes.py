"""The map sizes at which the engine branches on the map's geometry, one row per side of every threshold, and an
action stream whose offsets reach past every field that holds a coordinate.  Every test map before this table was
128 cells a side or less and every offset within [-2, 2]; zs_create accepts 16 000 cells a side, 2^24 cells in all,
and any int32 offset.  The thresholds (read from the headers as they stand):

  * closest_in (csrc/zs_tick.hpp): the packed-key minimum (d^2 << 16 | rank << 8 | slot) while
    (W-1)^2 + (H-1)^2 < 65536, else the three-way compare: 182 x 182 (largest d^2 65 522) | 183 x 182, 256 x 2 |
    257 x 2;
  * step_layout (csrc/zs_step_plan.hpp): the tick's spawn candidates in LDS (u16 entries) while W * H <= 65535,
    else in HBM: 255 x 257 | 256 x 256;
  * the widest and the tallest map validate() (csrc/engine.hip) admits, 16 000 x 1 and 1 x 16 000, and what it
    refuses (REFUSED);
  * the observation plan (csrc/zs_obs_plan.hpp): k_obs_patch and the ring's padded-table encoders while
    (W + 20) * 21 < 65536 and H < 4096: 3 100 x 1 | 3 101 x 1 (int16 and int64), 1 x 4 095 | 1 x 4 096;
    Dev::w_m (csrc/engine.hip: c / W by a multiply-shift) while W * H * W < 2^20: 255 x 16 | 256 x 16.
    The plan's LDS bound on k_obs_patch's padded table ((W + 20) * (H + 20) cells of 2 B beside eight waves'
    regions, 160 KiB in all) is met long before either geometric bound: 3 100 x 1 pads to 65 520 cells (131 KB)
    and 1 x 4 095 to 86 415, so all four strips take the select encoders (int64) or k_obs_pipe (int16), and the
    geometric conditions are never the ones that decide.  The rows stay: they are the longest rows and columns
    the 16-bit offsets and 12-bit obstacle coordinates were sized for, with windows over the padding at both ends.

Every row is a generated open field (geo_map): explicit spawn lists, and a few walls 3, 4, 10 and 11 cells from
the player spawn cells along the axes, so that the far stream's attacks and heals find something exactly at a
rifle's (10) and a heal's (3) range and one cell past it.  What a row claims (its `closest` side, `cand` side per
respawn variant, the lanes per env the plan resolves each requested G to, the observation kernels, `w_m`) is held
to the compiled plans and to the oracle's own run of the row by test_geometry_plan.py on the CPU; test_geometry.py
runs every row on the GPU against the oracle.

The closest rows.  The zombie spawn list is one corner and the player spawn list exactly the four players' cells,
two of them equidistant from that corner and nearer than the other two, so a zombie's first decision is a tie at
the minimum that dict rank decides, at a d^2 whose top bits are set.  On 182 x 182 the only cells at (0, 1)'s
and (1, 0)'s distance or farther from (181, 181) are those two and (0, 0), one short of four players: the tie at
the minimum is (0, 2) | (2, 0) (d^2 64 802) with (0, 1) | (1, 0) (65 161) behind it.  On 183 x 182 it is (1, 1) |
(2, 0) (65 161) with (1, 0) (65 522) and (0, 0) (65 885, the only d^2 >= 65536 of the map: the decisions of whoever
stands there) behind.  The two-row strips have no far tie (two cells of a strip are equidistant from a third only
next to it); on 257 x 2 the cells (0, 1) and (0, 0) are at 65 536 and 65 537 from the corner, whose low 16 bits
would beat every other key.
"""
import numpy as np

from libzombsole_amd import _abi
from libzombsole_amd import actions as A
from libzombsole_amd.maps import Map

STEPS, EPISODE = 24, 5
ENVS = (13, 37)
GS = (1, 8, 64)
I32_MAX, I32_MIN = (1 << 31) - 1, -(1 << 31)
RIFLE_RANGE, HEAL_RANGE = 10, 3


def closest_side(W, H):
    """closest_in's predicate (csrc/zs_tick.hpp)."""
    return "packed" if (W - 1) * (W - 1) + (H - 1) * (H - 1) < 65536 else "generic"


def w_m(W, H):
    """Dev::w_m as zs_create computes it (csrc/engine.hip): 0 = the divide."""
    return ((1 << 20) + W - 1) // W if W * H * W < (1 << 20) else 0


def patch_admitted(W, H):
    """The observation plan's geometry condition for k_obs_patch and the patched ring (csrc/zs_obs_plan.hpp)."""
    return (W + 20) * 21 < 65536 and H < 4096


# -- maps ------------------------------------------------------------------------------------------------------------
def geo_map(W, H, players, zombies, name, extra_walls=()):
    """An open W x H field: the player and zombie spawn lists as given, and walls 3, 4, 10 and 11 cells from every
    player spawn cell along both axes, towards the inside of the map (where that is on the map and no spawn cell),
    in row-major order."""
    taken = set(players) | set(zombies)
    walls = set(extra_walls)
    for px, py in players:
        sx = 1 if px < W // 2 else -1
        sy = 1 if py < H // 2 else -1
        for e in (HEAL_RANGE, HEAL_RANGE + 1, RIFLE_RANGE, RIFLE_RANGE + 1):
            for c in ((px + e * sx, py), (px, py + e * sy)):
                if 0 <= c[0] < W and 0 <= c[1] < H and c not in taken:
                    walls.add(c)
    walls = sorted(walls, key=lambda c: (c[1], c[0]))
    assert not (set(walls) & taken)
    return Map((W, H), [(x, y, _abi.THING_WALL) for x, y in walls], list(players), list(zombies), [], name=name)


def map_text(m):
    """The map as a map file's text ('w' wall, 'p' / 'z' spawn cells, '.' free): what the reference parses.  A
    parse lists the spawn cells in row-major order, whatever order the Map held them in."""
    W, H = m.size
    rows = [["."] * W for _ in range(H)]
    for cells, ch in ((m.obstacles, "w"), (m.player_spawns, "p"), (m.zombie_spawns, "z")):
        for c in cells:
            assert rows[c[1]][c[0]] == ".", c
            rows[c[1]][c[0]] = ch
    return "".join("".join(r) + "\n" for r in rows)


# the maps of the reference fixtures geo_* (tests/golden/make_golden.py), by the map name their kwargs hold; the file
# is written to a temporary directory when a fixture is recorded or replayed (golden_util.map_path)
FIXTURE_MAPS = {"geo183x182": lambda: closest_map(183, 182), "geo257x2": lambda: closest_map(257, 2),
                "geo16000x1": lambda: extreme_map(16000, 1)}


def _cfg(n, m, bots, initial, minimum, width=5, dtype=_abi.DTYPE_I64, rules="survival"):
    return _abi.multi_env_config(n, rules, bots, m, ["0", "1"], initial_zombies=initial, minimum_zombies=minimum,
                                 observation_surroundings_width=width, obs_dtype=dtype, agent_weapons="rifle",
                                 max_episode_steps=EPISODE)


CLOSEST_PLAYERS = {(182, 182): [(0, 2), (2, 0), (0, 1), (1, 0)], (183, 182): [(1, 1), (2, 0), (0, 0), (1, 0)],
                   (256, 2): [(0, 0), (0, 1), (1, 0), (1, 1)], (257, 2): [(0, 0), (0, 1), (1, 0), (1, 1)]}


def closest_map(W, H):
    return geo_map(W, H, CLOSEST_PLAYERS[(W, H)], [(W - 1, H - 1)], "geo%dx%d" % (W, H))


def _closest(W, H):
    # two zombies kept up from one spawn cell: one at the reset, the other as soon as the first has left it
    return lambda n: _cfg(n, closest_map(W, H), ["sniper", "terminator"], 1, 2)


def cand_map(W, H):
    """The zombie spawn list is the last three cells of the last row (the largest cell indices there are); the
    players stand ten rows above it."""
    return geo_map(W, H, [(W - 2, H - 6), (W - 4, H - 6), (W - 6, H - 6), (W - 8, H - 6)],
                   [(W - 1, H - 1), (W - 2, H - 1), (W - 3, H - 1)], "geo%dx%d" % (W, H))


def _cand(W, H):
    return lambda n: _cfg(n, cand_map(W, H), ["sniper", "terminator"], 1, 3)


def extreme_map(W, H):
    """Players at both ends of the strip, zombies one from either end's players and in the middle."""
    if H == 1:
        ps = [(0, 0), (1, 0), (W - 1, 0), (W - 2, 0)]
        zs = [(20, 0), (W // 2, 0), (W - 21, 0)]
    else:
        ps = [(0, 0), (0, 1), (0, H - 1), (0, H - 2)]
        zs = [(0, 20), (0, H // 2), (0, H - 21)]
    return geo_map(W, H, ps, zs, "geo%dx%d" % (W, H))


def _extreme(W, H):
    return lambda n: _cfg(n, extreme_map(W, H), ["sniper", "terminator"], 2, 3)


def obs_map(W, H):
    """Zombies spawn in the last cell of the map and in the last cell of the first row (they die there under the
    rifles beside them and leave their bodies), a wall stands next to each, and the four players spawn within ten
    cells of the borders, so that every window hangs over the padding."""
    last, first_row_last = (W - 1, H - 1), (W - 1, 0)
    zs = [last] if H == 1 else [last, first_row_last]
    if H == 1:
        ps = [(3, 0), (6, 0), (W - 4, 0), (W - 7, 0)]
        walls = [(W - 2, 0)]
    elif W == 1:
        ps = [(0, 3), (0, 6), (0, H - 4), (0, H - 7)]
        walls = [(0, H - 2), (0, 1)]
        zs = [last, (0, 0)]
    else:
        ps = [(3, 2), (W - 4, 1), (W - 5, H - 2), (W - 3, H - 3)]
        walls = [(W - 2, H - 1), (W - 2, 0)]
    return geo_map(W, H, ps, zs, "geo%dx%d" % (W, H), extra_walls=walls)


def _obs(W, H, dtype):
    return lambda n: _cfg(n, obs_map(W, H), ["sniper", "terminator"], 1, 2, width=21, dtype=dtype)


# -- the rows --------------------------------------------------------------------------------------------------------
class Row(object):
    """make(n) -> the config.  variants: [(name, zs_launch overrides)] beside the requested G, kernel and par_exec.
    G: requested lanes per env -> the lanes per env the plan resolves it to (a larger G where the image of 64 / G
    envs does not fit).  cand: variant name -> "lds" / "hbm".  obs: (obs_kernel, obs_kernel_masked, obs_encoders)
    or None where the row is no observation row (then describe()'s names are not part of the claim)."""
    stream = "far"

    def __init__(self, rid, W, H, make, closest, cand, G, variants, obs=None, wm=None, launch=None):
        self.id, self.W, self.H, self.make = rid, W, H, make
        self.closest, self.cand, self.G, self.variants, self.obs = closest, cand, G, variants, obs
        self.wm_zero = wm
        self.launch = dict(launch or {})
        self.seed0 = None

    def seeds(self, n):
        return [self.seed0 + i for i in range(n)]

    def builder(self, n, G=0, kernel="k_tick", par_exec=1, variant=None):
        b = self.make(n)
        b.cfg.lanes_per_env = G
        ov = dict(self.launch, fobs=-1, fused=1 if kernel == "k_step" else -1, par_exec=par_exec)
        ov.update(dict(self.variants)[variant] if variant else {})
        return b.set_launch(ov)

    def actions(self, seeds, t, n_agents):
        """The far stream at step t as the batched ABI takes it: int32 [len(seeds)][n_agents][3]."""
        return np.array([[A.encode_action(far_action(s, t, a, self.W, self.H)) for a in range(n_agents)]
                         for s in seeds], dtype=np.int32)


V_LEADER = ("leader", {"defer_respawn": -1})
V_KRESPAWN = ("k_respawn", {"defer_respawn": 1})
BOTH = [V_LEADER, V_KRESPAWN]
_LDS = {"leader": "lds", "k_respawn": "lds"}
_HBM = {"leader": "hbm", "k_respawn": "hbm"}
# the strips' and the 4 096-cell maps' bitmaps fit 64 to an image: the requested G stands; of the 33 124-cell bitmaps
# (4 KiB an env) eight fit, of the 65 535-cell ones (8 KiB) four, of the 16 000-cell ones sixteen
_G_ASKED = {1: 1, 8: 8, 64: 64}
OBS_LAUNCH = {"obs_lds": 1}  # the staged store kernels at any env count (int64 blocks take them from 12 288 envs)

ROWS = [
    Row("c182x182", 182, 182, _closest(182, 182), "packed", _LDS, {1: 8, 8: 8, 64: 64}, BOTH),
    Row("c183x182", 183, 182, _closest(183, 182), "generic", _LDS, {1: 8, 8: 8, 64: 64}, BOTH),
    Row("c256x2", 256, 2, _closest(256, 2), "packed", _LDS, _G_ASKED, BOTH),
    Row("c257x2", 257, 2, _closest(257, 2), "generic", _LDS, _G_ASKED, BOTH),
    Row("n255x257", 255, 257, _cand(255, 257), "generic", _LDS, {1: 16, 8: 16, 64: 64}, BOTH),
    Row("n256x256", 256, 256, _cand(256, 256), "generic", _HBM, {1: 16, 8: 16, 64: 64}, BOTH),
    Row("x16000x1", 16000, 1, _extreme(16000, 1), "generic", _LDS, {1: 4, 8: 8, 64: 64}, BOTH),
    Row("x1x16000", 1, 16000, _extreme(1, 16000), "generic", _LDS, {1: 4, 8: 8, 64: 64}, BOTH),
    Row("o3100x1_i16", 3100, 1, _obs(3100, 1, _abi.DTYPE_I16), "generic", _LDS, _G_ASKED, BOTH[:1],
        obs=("k_obs_pipe", "k_obs", ""), launch=OBS_LAUNCH),
    Row("o3100x1_i64", 3100, 1, _obs(3100, 1, _abi.DTYPE_I64), "generic", _LDS, _G_ASKED, BOTH[:1],
        obs=("k_obs_ring", "k_obs", "select"), launch=OBS_LAUNCH),
    Row("o3101x1_i16", 3101, 1, _obs(3101, 1, _abi.DTYPE_I16), "generic", _LDS, _G_ASKED, BOTH[:1],
        obs=("k_obs_pipe", "k_obs", ""), launch=OBS_LAUNCH),
    Row("o3101x1_i64", 3101, 1, _obs(3101, 1, _abi.DTYPE_I64), "generic", _LDS, _G_ASKED, BOTH[:1],
        obs=("k_obs_ring", "k_obs", "select"), launch=OBS_LAUNCH),
    Row("o1x4095", 1, 4095, _obs(1, 4095, _abi.DTYPE_I64), "generic", _LDS, _G_ASKED, BOTH[:1],
        obs=("k_obs_ring", "k_obs", "select"), launch=OBS_LAUNCH),
    Row("o1x4096", 1, 4096, _obs(1, 4096, _abi.DTYPE_I64), "generic", _LDS, _G_ASKED, BOTH[:1],
        obs=("k_obs_ring", "k_obs", "select"), launch=OBS_LAUNCH),
    Row("o255x16", 255, 16, _obs(255, 16, _abi.DTYPE_I64), "packed", _LDS, _G_ASKED, BOTH[:1],
        obs=("k_obs_ring", "k_obs", "patched"), wm=False, launch=OBS_LAUNCH),
    Row("o256x16", 256, 16, _obs(256, 16, _abi.DTYPE_I64), "packed", _LDS, _G_ASKED, BOTH[:1],
        obs=("k_obs_ring", "k_obs", "patched"), wm=True, launch=OBS_LAUNCH),
]
# first seeds: 61000 + 100 * the row's place, plus the first multiple of 7 at which the oracle's run of 37 envs holds
# every offset class with each of move, attack and heal and an attack and a heal at and just past their range
# (test_geometry_plan.py states the conditions; they were searched with the oracle alone)
_SEED_SHIFT = {"c183x182": 7, "n255x257": 28, "n256x256": 28, "x1x16000": 7, "o3100x1_i64": 28, "o3101x1_i16": 105,
               "o1x4095": 49, "o1x4096": 7, "o256x16": 14}
for _i, _r in enumerate(ROWS):
    _r.seed0 = 61000 + 100 * _i + _SEED_SHIFT.get(_r.id, 0)
BY_ID = {r.id: r for r in ROWS}


# -- what zs_create refuses --------------------------------------------------------------------------------------------
MSG_SIZE = "map size out of range"
MSG_STEP = "entity table / map too large for the LDS image of one env"
MSG_OBS = "map too large for the observation kernel's LDS image"


def _bare(W, H):
    """A W x H map with no obstacle and no spawn list (every cell a spawn candidate)."""
    return Map((W, H), [], [], [], [], name="bare%dx%d" % (W, H))


def _refuse_world(n):
    # a world-scope observation of 1 040 x 1 040 cells: the dead-body row alone (one bit a cell) is 135 KB
    return _abi.single_env_config(n, "survival", [], _bare(1040, 1040), "0", initial_zombies=1,
                                  observation_scope="world", observation_position_encoding="channels",
                                  max_episode_steps=EPISODE)


def _refuse_tick(n):
    # 254 entities on 690 x 700 cells: the observation image (no window map, no staged HP) still fits 64 KiB, the
    # tick image of a single env (G = 64: a 60 376-B bitmap and 15 B and more per entity) does not
    return _cfg(n, geo_map(690, 700, [(0, 0), (1, 0)], [(9, 9)], "geo690x700"), [], 200, 252)


# id -> (config builder, the message; "plan": which compiled plan states it, None = validate() / zs_create itself)
REFUSED = {
    "w16001": (lambda n: _cfg(n, _bare(16001, 1), [], 1, 0), MSG_SIZE, None),
    "h16001": (lambda n: _cfg(n, _bare(1, 16001), [], 1, 0), MSG_SIZE, None),
    "cells_2p24": (lambda n: _cfg(n, _bare(4097, 4096), [], 1, 0), MSG_SIZE, None),
    # no spawn lists: the reset image holds one candidate word per cell (200 x 205 = 41 000 cells, 164 000 B past
    # 160 KiB).  The step plan refuses it first: its fused image is the larger of the tick's and the reset's, and
    # with no fused image under 64 KiB at any G step_plan() gives up before it tries the unfused launch, so
    # zs_create's own 160 KiB message is never reached.
    "reset_image": (lambda n: _cfg(n, _bare(200, 205), [], 1, 0), MSG_STEP, "step"),
    "world_obs": (_refuse_world, MSG_OBS, "obs"),
    "tick_image": (_refuse_tick, MSG_STEP, "step"),
}


# -- the far action stream -------------------------------------------------------------------------------------------
# per axis: 14 of 20 draws from NEAR (0 six times in its 24 slots, so that an axis-aligned offset is common), 6 of 20
# from far(W or H).  Both axes near, so the target within a rifle's reach or one cell past it: (14 / 20)^2 = 49 %.
NEAR = [0] * 6 + [1, -1, 2, -2, 9, -9] + [3, -3, 4, -4, 10, -10, 11, -11] + [3, 4, 10, 11]


def far_offsets(extent):
    """The offsets past a rifle's reach for an axis of `extent` cells: the map's own size, either side of the
    clamp (16 384), of int16 and of 16 bits, and the ends of int32."""
    out = []
    for v in (extent - 1, extent, 16383, 16384, 16385, 32767, 32768, 65535, 65536, 65537):
        out += [v, -v]
    return out + [I32_MAX, I32_MIN]


def offset_classes(extent):
    """name -> the offsets of one class (the CPU test wants every class with each of move, attack and heal)."""
    c = {"0": [0], "1": [1, -1], "2": [2, -2], "9": [9, -9], "10": [10, -10], "11": [11, -11]}
    for name, v in (("W-1", extent - 1), ("W", extent), ("16383", 16383), ("16384", 16384), ("16385", 16385),
                    ("32767", 32767), ("32768", 32768), ("65535", 65535), ("65536", 65536), ("65537", 65537)):
        c.setdefault(name, [v, -v])
    c["int32_max"], c["int32_min"] = [I32_MAX], [I32_MIN]
    return c


def _axis(h, extent, beyond):
    far = far_offsets(extent) + ([1 << 40, -(1 << 40)] if beyond else [])
    if h % 20 < 14:
        return NEAR[(h >> 5) % len(NEAR)]
    return far[(h >> 5) % len(far)]


def far_action(seed, step, agent, W, H, beyond=False):
    """rich_action's kinds with offsets drawn per axis from {0, +-1, +-2, +-9, +-10, +-11, +-(W-1), +-W, +-16 383,
    +-16 384, +-16 385, +-32 767, +-32 768, +-65 535, +-65 536, +-65 537, 2^31 - 1, -2^31} (H for W on the y axis),
    and +-3, +-4 beside them: a heal reaches 3 cells whatever the weapon, so the stream's own set holds no heal at
    or just past its range.  beyond: also +-2^40, as Python ints (the reference's fixtures)."""
    h = A.action_hash(seed, step, agent)
    atype = A.RICH_TYPES[h % 8]
    dx = _axis(h >> 8, W, beyond)
    dy = _axis(h >> 32, H, beyond)
    return {"action_type": atype, "parameter": [dx, dy]}


# -- the oracle's own run of a row -----------------------------------------------------------------------------------
def _d2(ax, ay, bx, by):
    return (ax - bx) ** 2 + (ay - by) ** 2


def oracle_census(row, n, steps=STEPS):
    """The oracle alone over the row's config, seeds, stream and steps.  Returns per env a dict of counts, taken
    from the state before every step: closest decisions (every zombie's closest player; every sniper's,
    terminator's and attack_closest agent's closest zombie; every heal_closest agent's closest other player) by
    the d^2 of the minimum ("far" >= 65 536, "high" >= 60 000) and ties at the minimum; the steps at which a zombie
    or a body lies in the last cell of the map ("last_cell") or of the first row ("row_end") within an agent's
    window; and, per kind of action,
    the offset classes seen and the attacks and heals on a thing at exactly their range and one cell past it."""
    from oracle.oracle import OracleEnv
    cls = {"x": offset_classes(row.W), "y": offset_classes(row.H)}
    out = []
    for s in row.seeds(n):
        o = OracleEnv(row.make(1))
        o.seed(s)
        o.reset()
        c = {"far": 0, "high": 0, "ties": 0, "far_ties": 0, "decisions": 0, "classes": set(), "edge": set(),
             "autoresets": 0, "respawns": 0, "last_cell": 0, "row_end": 0}
        need = False
        bots = [int(b) for b in o.builder.cfg.bot_types[:o.builder.num_bots]]
        occupied = {(ob[0], ob[1]) for ob in o.builder.map.obstacles}
        for t in range(1, steps + 1):
            if need:
                o.reset()
                need = False
                c["autoresets"] += 1
                continue
            acts = row.actions([s], t, o.A)[0]
            st = o.state()
            zs = [(d[1], d[2]) for d in st["dyn"] if d[0] == _abi.THING_ZOMBIE]
            ps = [(d[1], d[2], d[0], d[5]) for d in st["dyn"] if d[0] in (_abi.THING_PLAYER, _abi.THING_AGENT)]

            def decide(fx, fy, others):
                if not others:
                    return
                ds = sorted(_d2(fx, fy, x, y) for x, y in others)
                c["decisions"] += 1
                c["far"] += ds[0] >= 65536
                c["high"] += ds[0] >= 60000
                tie = len(ds) > 1 and ds[0] == ds[1]
                c["ties"] += tie
                c["far_ties"] += tie and ds[0] >= 60000
            for zx, zy in zs:
                decide(zx, zy, [(p[0], p[1]) for p in ps])
            things = occupied | set(zs) | {(p[0], p[1]) for p in ps}
            # a zombie or a body in the last cell of the map / of the first row, inside an agent's 21-cell window
            shown = set(zs) | {(d % row.W, d // row.W) for d in st["dead"]}
            for key, cell in (("last_cell", (row.W - 1, row.H - 1)), ("row_end", (row.W - 1, 0))):
                c[key] += cell in shown and any(p[2] == _abi.THING_AGENT and abs(p[0] - cell[0]) <= 10 and
                                                abs(p[1] - cell[1]) <= 10 for p in ps)
            for px, py, kind, extra in ps:
                if kind == _abi.THING_PLAYER:
                    if bots[extra] in (_abi.BOT_SNIPER, _abi.BOT_TERMINATOR):
                        decide(px, py, zs)
                    continue
                k, dx, dy = (int(v) for v in acts[extra])
                if k == A.ACT_ATTACK_CLOSEST:
                    decide(px, py, zs)
                elif k == A.ACT_HEAL_CLOSEST:
                    decide(px, py, [(q[0], q[1]) for q in ps if (q[0], q[1]) != (px, py)])
                name = {A.ACT_MOVE: "move", A.ACT_ATTACK: "attack", A.ACT_HEAL: "heal"}.get(k)
                if not name:
                    continue
                for axis, v in (("x", dx), ("y", dy)):
                    for cn, vals in cls[axis].items():
                        if v in vals:
                            c["classes"].add((name, cn))
                if name != "move" and (px + dx, py + dy) in things and (dx, dy) != (0, 0):
                    r2 = dx * dx + dy * dy
                    reach = RIFLE_RANGE if name == "attack" else HEAL_RANGE
                    if name == "heal" and (px + dx, py + dy) in zs:
                        continue  # a zombie is never healed
                    if r2 == reach * reach:
                        c["edge"].add((name, "at"))
                    elif reach * reach < r2 <= (reach + 1) * (reach + 1):
                        c["edge"].add((name, "past"))
            _, _, d, tr, _ = o.step(acts)
            need = d or tr
        c["respawns"] = o.census().get("respawns", 0)
        out.append(c)
    return out
