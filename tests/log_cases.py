"""The case table of the action and death logs (ZS_FLAG_DEATH_LOG: zs_action_log, zs_death_log): one row per
step-kernel instantiation, G in {1 .. 64} x {k_step, k_tick5, k_tick6}, on step_instantiations.Row (its launch
overrides, its env counts 67 / 37 / 13 with a partial last workgroup, its action streams), each with the flag
or-ed in and with zombie counts and episode lengths under which things die within the 24 steps; and three rows on
a debug config whose stream holds ZS_ACT_RAISE.  test_log_plan.py counts on the CPU, with the oracle alone, the
classes of CLASSES per row and requires that the rows of every G meet each of them NEED_EACH times between them
(or name it in UNREACHABLE with the reason); test_logs.py runs every row on the GPU and compares both logs of every
env at every step with the oracle's.

Which piece of zs_tick.hpp writes a step's action log follows the list: the env's G lanes execute (and log) a
list of at most 2G actions none of whose decisions drew from the stream, in chunks of G; the leader's serial loop
takes (and logs) every other list; a debug raise is logged by the leader where it stops.  The death log is written
by env_cleanup_group<G>, which walks the K things of the pre-step dict order and then the step's successful movers
in execution order, G entries a chunk (walk() below): a thing that moved is skipped at its old place and met
again behind the K, which is the order the reference's dict gives (core.py:158-159, 121-138).
"""
import numpy as np

from libzombsole_amd import _abi
from libzombsole_amd import actions as A
from libzombsole_amd.maps import Map

import step_instantiations as S
from test_conflict_census import MELEE_MAP

STEPS = S.STEPS
NEED_EACH = 3


def _multi(n, rules, bots, map_, agents, zombies, weapons, episode, minimum=None, debug=False):
    b = _abi.multi_env_config(n, rules, bots, map_, [str(i) for i in range(agents)], initial_zombies=zombies,
                              minimum_zombies=zombies if minimum is None else minimum, agent_weapons=weapons,
                              max_episode_steps=episode, debug=debug)
    b.cfg.flags |= _abi.FLAG_DEATH_LOG
    return b


def _pen():
    return Map.from_text(S.PEN_MAP, name="pen")


def _melee():
    return Map.from_text(MELEE_MAP, name="melee")


# the melee map with six player spawns: room for bots beside the agents
PIT_MAP = ("wwwwwwwwwwww\n"
           "w.pppppp...w\n"
           "w.zzzzzzzz.w\n"
           "w.zzzzzzzz.w\n"
           "w..........w\n"
           "wwwwwwwwwwww\n")


def _pit():
    return Map.from_text(PIT_MAP, name="pit")


# no zombie spawns listed: a zombie spawns on any free cell of the 72, more than 64, so the respawn is k_respawn's
ARENA_MAP = ("wwwwwwwwwwww\n"
             "w..pppp....w\n"
             "w..........w\n"
             "w..........w\n"
             "w..........w\n"
             "wwwwwwwwwwww\n")
# 80 zombie spawns (k_respawn) and six player spawns
HORDE_MAP = ("wwwwwwwwwwwwwwwwwwwwww\n"
             "w.pppppp.............w\n"
             "w.zzzzzzzzzzzzzzzzzzzz\n"
             "w.zzzzzzzzzzzzzzzzzzzz\n"
             "w.zzzzzzzzzzzzzzzzzzzz\n"
             "w.zzzzzzzzzzzzzzzzzzzz\n"
             "w....................w\n"
             "wwwwwwwwwwwwwwwwwwwwww\n")


def arena(n):
    """Two agents and three zombies that respawn anywhere (k_respawn on a map small enough for G = 1)."""
    return _multi(n, "survival", [], Map.from_text(ARENA_MAP, name="arena"), 2, 3, ["shotgun", "axe"], 12)


def horde75(n):
    """81 things shoulder to shoulder: lists and cleanup walks of more than 64 entries, many removals a step."""
    return _multi(n, "survival", ["terminator", "troll"], Map.from_text(HORDE_MAP, name="horde"), 4, 75,
                  ["shotgun", "axe", "shotgun", "rifle"], 12)


def lonely(n):
    """Two agents and nothing else under survival rules: the rich stream's idle agents give empty lists."""
    return _multi(n, "survival", [], _pen(), 2, 0, ["axe", "gun"], 6)


def pen_duo(n):
    return _multi(n, "extermination", [], _pen(), 1, 1, ["axe"], 8)


def pen_quad(n):
    return _multi(n, "extermination", [], _pen(), 2, 2, ["axe", "shotgun"], 8)


def pen_six(n):
    return _multi(n, "extermination", [], _pen(), 2, 4, ["axe", "shotgun"], 8)


def pen_ham(n):
    return _multi(n, "extermination", ["hamster"], _pen(), 1, 2, ["axe"], 8)


def brawl(n):
    """Two agents with shotguns among seven zombies on the crowded melee map."""
    return _multi(n, "survival", [], _melee(), 2, 7, ["shotgun", "axe"], 12)


def melee(n):
    """Four agents among fourteen zombies: agents die, and zombies by the dozen."""
    return _multi(n, "survival", [], _melee(), 4, 14, ["shotgun", "axe", "shotgun", "rifle"], 12)


def melee_bots(n):
    """The melee with a hamster (a deferred decision), a troll and a terminator among the zombies: bots die."""
    return _multi(n, "survival", ["hamster", "troll", "terminator"], _pit(), 2, 12, ["shotgun", "axe"], 12)


def fort(n):
    """fort lists 600 zombie spawns: the respawn is k_respawn's."""
    return _multi(n, "survival", ["hamster", "terminator", "troll"], "fort", 3, 12, ["shotgun", "gun", "axe"], 12)


def city(n, zombies=50):
    """city128 lists 439 zombie spawns (k_respawn); rifles and shotguns kill often."""
    return _multi(n, "safehouse", [], "city128", 4, zombies, ["rifle", "shotgun", "rifle", "gun"], 12)


def city70(n):
    return city(n, 70)


def city140(n):
    return city(n, 140)


def raise_pen(n):
    """debug = True: an agent whose action is ZS_ACT_RAISE stops the step (core.py:96-99)."""
    return _multi(n, "survival", [], _pen(), 3, 3, ["axe", "gun", "knife"], 8, debug=True)


def raise_ham(n):
    """... behind a hamster in dict order, whose decision drew from the stream before the raise."""
    return _multi(n, "survival", ["hamster", "troll"], _pit(), 3, 8, ["axe", "gun", "knife"], 8, debug=True)


# config -> (builder, action stream, describe()'s respawn).  "bad" is actions.bad_action: the rich stream with one
# action in eight carrying a parameter Agent.next_step raises on, ZS_ACT_RAISE under debug.
CONFIGS = {"lonely": (lonely, "rich", "tick"), "pen_duo": (pen_duo, "rich", "tick"), "pen_quad": (pen_quad, "rich", "tick"),
           "pen_six": (pen_six, "rich", "tick"), "pen_ham": (pen_ham, "rich", "tick"), "brawl": (brawl, "rich", "tick"),
           "melee": (melee, "discrete", "tick"), "melee_rich": (melee, "rich", "tick"),
           "melee_bots": (melee_bots, "rich", "tick"), "fort": (fort, "rich", "k_respawn"),
           "city": (city, "discrete", "k_respawn"), "city70": (city70, "discrete", "k_respawn"),
           "city140": (city140, "discrete", "k_respawn"),
           "arena": (arena, "rich", "k_respawn"), "horde75": (horde75, "discrete", "k_respawn"),
           "raise_pen": (raise_pen, "bad", "tick"), "raise_ham": (raise_ham, "bad", "tick")}


class LogRow(S.Row):
    def __init__(self, G, kernel, config, n=None, tag=""):
        self.G, self.kernel, self.config, self.regimes = G, kernel, config, ()
        self.n = S.ENVS[G] if n is None else n
        self.make, self.stream, self.respawn = CONFIGS[config]
        launch, self.step_kernel, self.tick_waves = S.KERNEL_LAUNCH[kernel]
        self.launch = dict(launch, fobs=-1)
        self.fused = kernel == "k_step"
        self.seed0 = 21000 + 100 * G + 1000 * S.KERNELS.index(kernel)
        self.id = "G%d-%s-%s@%d%s" % (G, kernel, config, self.n, tag)

    def actions(self, seeds, t, n_agents):
        if self.stream != "bad":
            return S.Row.actions(self, seeds, t, n_agents)
        out = np.zeros((len(seeds), n_agents, 3), dtype=np.int32)
        for i, s in enumerate(seeds):
            for a in range(n_agents):
                try:
                    out[i, a] = A.encode_action(A.bad_action(s, t, a))
                except A.ActionError:
                    out[i, a] = (A.ACT_RAISE, 0, 0)
        return out


_ROWS = {
    (1, "k_step"): "arena", (1, "k_tick5"): "melee_bots", (1, "k_tick6"): "lonely",
    (2, "k_step"): "arena", (2, "k_tick5"): "melee_bots", (2, "k_tick6"): "lonely",
    (4, "k_step"): "brawl", (4, "k_tick5"): "melee_bots", (4, "k_tick6"): "arena",
    (8, "k_step"): "melee", (8, "k_tick5"): "arena", (8, "k_tick6"): "melee_bots",
    (16, "k_step"): "melee_rich", (16, "k_tick5"): "city", (16, "k_tick6"): "melee_bots",
    (32, "k_step"): "city", (32, "k_tick5"): "melee_bots", (32, "k_tick6"): "horde75",
    (64, "k_step"): "horde75", (64, "k_tick5"): "melee_bots", (64, "k_tick6"): "city140",
}
ROWS = [LogRow(G, k, cfg) for (G, k), cfg in _ROWS.items()]
# empty lists at the lane counts whose three rows hold none: a few envs of the lonely config, less than one workgroup
# at G = 4 and 8, more than one from G = 16
EMPTY_ROWS = [LogRow(4, "k_tick5", "lonely", 5, "-empty"), LogRow(8, "k_tick6", "lonely", 5, "-empty"),
              LogRow(16, "k_step", "lonely", 5, "-empty"), LogRow(32, "k_tick5", "lonely", 3, "-empty"),
              LogRow(64, "k_step", "lonely", 3, "-empty")]
# the debug rows: a few envs each, at every lane count; the G = 8 one with a hamster before the agents
RAISE_ROWS = [LogRow(1, "k_tick5", "raise_pen", 5, "-raise"), LogRow(2, "k_step", "raise_pen", 5, "-raise"),
              LogRow(4, "k_tick6", "raise_pen", 5, "-raise"), LogRow(8, "k_step", "raise_ham", 11, "-raise"),
              LogRow(8, "k_tick5", "raise_pen", 5, "-raise"), LogRow(16, "k_tick6", "raise_pen", 5, "-raise"),
              LogRow(32, "k_step", "raise_pen", 3, "-raise"), LogRow(64, "k_tick6", "raise_pen", 3, "-raise")]
ALL_ROWS = ROWS + EMPTY_ROWS + RAISE_ROWS

LIST_CLASSES = ("empty", "one_chunk", "two_chunk", "serial_long", "deferred", "void", "obst_target", "raise_k0",
                "raise_kpos")
REMOVAL_CLASSES = ("multi", "two_chunks", "moved", "agent", "bot", "reuse_tick", "reuse_k_respawn")
CLASSES = LIST_CLASSES + REMOVAL_CLASSES

# G -> {class: why no row of that G can meet it}
UNREACHABLE = {}


def walk(pre_cells, alog_rows):
    """The cleanup's walk of a step: the pre-step cell of the thing at every walk index, the K things of the
    pre-step dict order, then the successful movers in execution order (a mover is listed twice; the cleanup skips
    it at its first place)."""
    return list(pre_cells) + [r[0] for r in alog_rows if r[2] == 1 and r[4]]


def walk_index(pre_cells, alog_rows, cell):
    """The walk index at which the cleanup meets the thing that stood on `cell` before the step."""
    movers = [r[0] for r in alog_rows if r[2] == 1 and r[4]]
    return len(pre_cells) + movers.index(cell) if cell in movers else list(pre_cells).index(cell)


def classify(G, n, rows, drew, deaths, pre, post, slots, respawn):
    """The classes (CLASSES) one step of the oracle meets at lanes-per-env G: its action log (n, rows, drew), its
    death log, the states before and after it, the config's zombie slots and its respawn ("tick", "k_respawn")."""
    got = set()
    if n < 0:
        got.add("raise_k0" if n == -1 else "raise_kpos")
        return got
    if n == 0:
        got.add("empty")
    elif n > 2 * G:
        got.add("serial_long")
    elif not drew:
        got.add("one_chunk" if n <= G else "two_chunk")
    if drew and n > 0:
        got.add("deferred")
    if any(not r[4] for r in rows):
        got.add("void")
    if any(r[3][0] == "obst" for r in rows):
        got.add("obst_target")
    if len(deaths) >= 2:
        got.add("multi")
    cells = [(d[1], d[2]) for d in pre["dyn"]]
    idx = [walk_index(cells, rows, d[5]) for d in deaths]
    if len({i // G for i in idx}) >= 2:
        got.add("two_chunks")
    if any(i >= len(cells) for i in idx):
        got.add("moved")
    if any(d[0] == _abi.THING_AGENT for d in deaths):
        got.add("agent")
    if any(d[0] == _abi.THING_PLAYER for d in deaths):
        got.add("bot")
    # every zombie slot is taken after the step: the respawn refilled the slot of every zombie the step removed
    if any(d[0] == _abi.THING_ZOMBIE for d in deaths) and sum(d[0] == _abi.THING_ZOMBIE for d in post["dyn"]) == slots:
        got.add("reuse_" + respawn)
    return got


def census(row, steps=STEPS):
    """How many steps of the row's run (its config, seeds, stream, autoresets) meet every class, by the oracle."""
    from oracle.oracle import OracleEnv, OracleRaised
    tot = dict.fromkeys(CLASSES + ("resets", "entries", "removed"), 0)
    cfg = row.make(1).cfg
    slots = max(cfg.initial_zombies, cfg.minimum_zombies)
    for s in row.seeds():
        o = OracleEnv(row.make(1))
        o.seed(s)
        o.reset()
        o.set_logs()
        need = False
        for t in range(1, steps + 1):
            if need:
                o.reset()
                need = False
                tot["resets"] += 1
                assert o.action_log()[0] == 0 and o.death_log() == []
                continue
            pre = o.state()
            try:
                _, _, d, tr, _ = o.step(row.actions([s], t, o.A)[0])
                need = d or tr
            except OracleRaised:
                pass
            n, rows, drew = o.action_log()
            deaths = o.death_log()
            tot["entries"] += len(rows)
            tot["removed"] += len(deaths)
            for c in classify(row.G, n, rows, drew, deaths, pre, o.state(), slots, row.respawn):
                tot[c] += 1
    return tot
