"""One case per step-kernel instantiation (libzombsole_amd/csrc/k_tick_g.hip, compiled for G = 1 .. 64 lanes per
env): k_step<G> (reset work and tick in one launch), k_tick<G, 5> and k_tick<G, 6> (the tick alone, compiled for
5 or 6 waves per SIMD): 21 device functions.  test_step_instantiations_plan.py checks on the CPU that the rows
and the UNREACHABLE dict together are the 21, that the compiled step plan resolves every row to its instantiation
(the LDS image of the requested G fits, so the plan does not raise the G) and, with the oracle's census, that the rows of every G meet the action-list regimes they
claim; test_step_instantiations.py runs every row on the GPU.

What describe() must report is what the compiled step plan (libzombsole_amd/csrc/zs_step_plan.hpp, through
tests/step_plan_dump.cpp) resolves every row's config and overrides to; test_step_instantiations_plan.py checks on
the CPU that this is the row's G, kernel and wave budget:

  * zs_launch.fused = 1 takes k_step at any env count, fused = -1 k_tick, whose register budget
    zs_launch.tick_waves (5 or 6) then names; describe()'s "tick_waves" is ZS_FUSED_WAVES (3) for k_step;
  * the plan starts at the requested G and doubles it only while no LDS image of 64 / G envs fits 64 KiB, not even
    the smallest one (a 32-word RNG window, no spawn-candidate copy, no spawn lists; min_image_args() below);
  * respawn by k_respawn where the config keeps a minimum of zombies and the zombie spawn list (or the map,
    without one) has more than 64 cells, by the tick otherwise (step_defer_respawn()); par_exec = 1 unless
    zs_launch.par_exec is -1.

Every row sets fobs = -1 (observations by the observation kernels, never by the step launch), so no observation
image enters the step's LDS arithmetic.

Env counts: the smallest with two or more workgroups and a partial last one (a workgroup holds 64 / G envs), see
ENVS; SMALL_ROWS are launches of less than one workgroup.  With 37 envs at G = 8 the tick grid is 5 workgroups
and the fused one 5 + 37, neither a multiple of 8 (xcd_remap).

Action-list regimes (zs_tick.hpp tick_wg / grp_execute): the env's G lanes execute a list of at most 2G actions
in chunks of G; the leader's serial loop takes longer lists and lists with a decision that drew from the stream
(hamster, randoman, a wandering zombie).  Every row names the regimes it provides; NEED what the rows of one G
must provide between them.
"""
import numpy as np

from libzombsole_amd import _abi
from libzombsole_amd import actions as A
from libzombsole_amd.maps import Map

from test_conflict_census import MELEE_MAP

GS = (1, 2, 4, 8, 16, 32, 64)
KERNELS = ("k_step", "k_tick5", "k_tick6")
# kernel -> (zs_launch overrides, describe()'s step_kernel, tick_waves)
KERNEL_LAUNCH = {"k_step": ({"fused": 1}, "k_step", 3),
                 "k_tick5": ({"fused": -1, "tick_waves": 5}, "k_tick", 5),
                 "k_tick6": ({"fused": -1, "tick_waves": 6}, "k_tick", 6)}
# G -> env count of its rows (64 / G envs per workgroup; the last workgroup holds 3, 5, 5, 5, 1, 1, 1)
ENVS = {1: 67, 2: 37, 4: 37, 8: 37, 16: 37, 32: 37, 64: 13}
STEPS, EPISODE = 24, 5  # every episode is truncated at 5 steps or earlier: four autoresets or more per env

# a small pen: boxes to bump into and to hit, four player and four zombie spawns, 60 cells (two bitmap words)
PEN_MAP = ("wwwwwwwwww\n"
           "wp.b....zw\n"
           "wp...b..zw\n"
           "w..b....zw\n"
           "wp.p.b..zw\n"
           "wwwwwwwwww\n")


def _pen(n, agents, bots, zombies):
    return _abi.multi_env_config(n, "extermination", bots, Map.from_text(PEN_MAP, name="pen"),
                                 [str(i) for i in range(agents)], initial_zombies=zombies, minimum_zombies=zombies,
                                 agent_weapons=["axe", "gun"], max_episode_steps=EPISODE)


def pen_duo(n):
    """One agent, one zombie kept alive by respawns: lists of one or two actions."""
    return _pen(n, 1, [], 1)


def pen_quad(n):
    """Two agents, two zombies: lists of up to four actions."""
    return _pen(n, 2, [], 2)


def pen_six(n):
    """Two agents, four zombies: lists of up to six actions."""
    return _pen(n, 2, [], 4)


def pen_ham(n):
    """An agent, a hamster (its move is a draw from the stream: a deferred decision) and a zombie."""
    return _pen(n, 1, ["hamster"], 1)


def c2(n):
    return _abi.multi_env_config(n, "extermination", [], "bridge64", ["0", "1"], initial_zombies=10,
                                 minimum_zombies=0, max_episode_steps=EPISODE)


def c5(n):
    return _abi.multi_env_config(n, "extermination", [], "bridge64", ["0", "1", "2", "3"], initial_zombies=20,
                                 obs_dtype=_abi.DTYPE_I16, max_episode_steps=EPISODE)


def c4(n):
    return _abi.multi_env_config(n, "safehouse", [], "city128", ["0", "1", "2", "3"], initial_zombies=50,
                                 minimum_zombies=50, max_episode_steps=EPISODE)


def melee(n):
    """The crowded 12 x 6 map of test_conflict_census.py under the random policy: 18 actors shoulder to shoulder."""
    return _abi.multi_env_config(n, "survival", [], Map.from_text(MELEE_MAP, name="melee"), ["0", "1", "2", "3"],
                                 initial_zombies=14, minimum_zombies=14, max_episode_steps=EPISODE)


def fort_bots(n):
    """The rich-action fort config of test_lanes_per_env (heals of others, hits on obstacles, bad parameters) with
    a hamster among the bots, whose moves are deferred decisions."""
    return _abi.multi_env_config(n, "survival", ["hamster", "terminator", "troll"], "fort", ["0", "1", "2"],
                                 initial_zombies=12, minimum_zombies=8, agent_weapons=["shotgun", "gun", "axe"],
                                 max_episode_steps=EPISODE)


def brawl9(n):
    """Nine entities on the crowded melee map: lists of seven to nine actions under the rich stream (an agent's
    action may come to nothing), on either side of 2G = 8 and of G = 8."""
    return _abi.multi_env_config(n, "survival", [], Map.from_text(MELEE_MAP, name="melee"), ["0", "1"],
                                 initial_zombies=7, minimum_zombies=7, agent_weapons=["shotgun", "knife"],
                                 max_episode_steps=EPISODE)


# config -> (builder, action stream, describe()'s respawn).  Streams: "discrete" is zs_gen_actions' (every agent
# acts at every step), "rich" is actions.rich_action (idle and void actions, hits on obstacles, heals of others,
# out-of-range parameters), so a list's length varies with the agents that act.  city128 lists 439 zombie spawns
# and fort 600
# (> 64: k_respawn); the pen lists 4, the melee map 16; c2 and c5 keep no minimum.
CONFIGS = {"pen_duo": (pen_duo, "rich", "tick"), "pen_quad": (pen_quad, "rich", "tick"),
           "pen_six": (pen_six, "rich", "tick"), "pen_ham": (pen_ham, "discrete", "tick"),
           "c2": (c2, "discrete", "tick"), "brawl9": (brawl9, "rich", "tick"), "c5": (c5, "discrete", "tick"),
           "c4": (c4, "discrete", "k_respawn"), "melee": (melee, "discrete", "tick"),
           "melee_rich": (melee, "rich", "tick"), "fort_bots": (fort_bots, "rich", "k_respawn")}

# (G, kernel) -> (config, the regimes the row claims, see REGIME_COUNTERS).  Entities: pen_duo 2, pen_ham 3,
# pen_quad 4, pen_six 6, brawl9 9, c2 12, melee 18, fort_bots 18, c5 24, c4 54.  A list holds one action per alive
# zombie and bot (they always act) and one per agent whose action comes to something.  Things do die within the
# five steps (the oracle counts 0 to 344 deaths a row), but next to nothing ends: of about 3 400 episodes two end
# by a rule (both in brawl9), every other one is the five-step truncation, and G = 1, 2, 16, 32 and 64 never see
# done = 1.  The ways an episode ends are the table of terminal_outcomes.py.
_ROWS = {
    # G = 1: chunks of one action; more than two actions go to the leader
    (1, "k_step"): ("pen_duo", ("one_chunk", "two_chunk")),
    (1, "k_tick5"): ("c2", ("serial_long",)),
    (1, "k_tick6"): ("pen_ham", ("deferred",)),
    # G = 2: up to four actions by the lanes
    (2, "k_step"): ("pen_ham", ("deferred",)),
    (2, "k_tick5"): ("pen_quad", ("one_chunk", "two_chunk")),
    (2, "k_tick6"): ("c2", ("serial_long",)),
    # G = 4: up to eight
    (4, "k_step"): ("brawl9", ("serial_long", "two_chunk")),
    (4, "k_tick5"): ("fort_bots", ("deferred", "serial_long")),
    (4, "k_tick6"): ("pen_six", ("one_chunk", "two_chunk")),
    # G = 8: up to sixteen
    (8, "k_step"): ("melee", ("serial_long",)),
    (8, "k_tick5"): ("brawl9", ("one_chunk", "two_chunk")),
    (8, "k_tick6"): ("fort_bots", ("deferred",)),
    # G = 16: up to thirty-two
    (16, "k_step"): ("melee_rich", ("one_chunk", "two_chunk")),
    (16, "k_tick5"): ("c4", ("serial_long",)),
    (16, "k_tick6"): ("fort_bots", ("deferred",)),
    # G = 32: a two-chunk row (33 to 64 actors); from here the lanes decide by slot class (agents, bots, zombies)
    (32, "k_step"): ("c4", ("two_chunk",)),
    (32, "k_tick5"): ("melee", ("one_chunk",)),
    (32, "k_tick6"): ("fort_bots", ("deferred",)),
    # G = 64: one chunk
    (64, "k_step"): ("c4", ("one_chunk",)),
    (64, "k_tick5"): ("fort_bots", ("deferred",)),
    (64, "k_tick6"): ("c5", ("one_chunk",)),
}
# launches of less than one workgroup, one per kernel kind: 3 of the 64 envs of a G = 1 workgroup (lists of two
# to four actions: both paths in one workgroup), 1 of the 4 of a G = 16 one
_SMALL = {(1, "k_step", 3): ("pen_quad", ("serial_long", "two_chunk")), (16, "k_tick6", 1): ("c2", ("one_chunk",))}

# Instantiations no config reaches, each with the step_plan() condition (zs_step_plan.hpp) that excludes it.  There is none: every G fits some config's image, fused = 1 / -1 forces k_step / k_tick at any env count and
# tick_waves forces either register budget.
UNREACHABLE = {}

# regime -> the census counters (oracle.CENSUS_EXT) that must be non-zero
REGIME_COUNTERS = {"one_chunk": ("lists", "lists_1chunk", "chunks"), "two_chunk": ("lists", "lists_2chunk", "chunks"),
                   "serial_long": ("lists_serial", "serial_long"), "deferred": ("lists_serial", "serial_drew")}
# what the rows of one G must provide between them
_ALL4 = ("one_chunk", "two_chunk", "serial_long", "deferred")
NEED = {1: _ALL4, 2: _ALL4, 4: _ALL4, 8: _ALL4, 16: _ALL4, 32: ("two_chunk",), 64: ("one_chunk",)}
# The conflict cases of the lanes' chunked execution (test_conflict_census.py) that the rows of one G must meet
# between them.  A chunk of one action (G = 1) holds no conflict; two small envs never put a hit on a body a hit
# of the same two-action chunk killed; the rich stream's moves are mostly longer than a step, so a move into a
# cell vacated in the same chunk needs the discrete stream's rows, which are on the lanes' path from G = 32 on.
# No obstacle is poked here: no obst_int16.
CONFLICTS = ("enter_vacated", "same_dest", "target_moved", "multi_hit", "hit_dead", "heal_clamp")
_CORE = ("same_dest", "target_moved", "multi_hit", "heal_clamp")
CONFLICTS_NEED = {1: (), 2: _CORE, 4: _CORE + ("hit_dead",), 8: _CORE + ("hit_dead",), 16: _CORE + ("hit_dead",),
                  32: CONFLICTS, 64: CONFLICTS}


class Row(object):
    def __init__(self, G, kernel, config, regimes, n=None):
        self.G, self.kernel, self.config, self.regimes = G, kernel, config, regimes
        self.n = ENVS[G] if n is None else n
        self.make, self.stream, self.respawn = CONFIGS[config]
        launch, self.step_kernel, self.tick_waves = KERNEL_LAUNCH[kernel]
        self.launch = dict(launch, fobs=-1)
        self.fused = kernel == "k_step"
        self.seed0 = 9000 + 100 * G + 1000 * KERNELS.index(kernel)
        self.id = "G%d-%s-%s@%d" % (G, kernel, config, self.n)

    def builder(self, n=None, par_exec=1):
        """The engine's config (n envs, the row's G and overrides), or with n = 1 and no override the oracle's."""
        b = self.make(self.n if n is None else n)
        b.cfg.lanes_per_env = self.G
        return b.set_launch(dict(self.launch, par_exec=par_exec))

    def seeds(self):
        return [self.seed0 + i for i in range(self.n)]

    def describe(self, par_exec=1):
        """The fields describe() must report."""
        return {"envs": self.n, "lanes_per_env": self.G, "step_kernel": self.step_kernel,
                "tick_waves": self.tick_waves, "par_exec": 1 if par_exec >= 0 else 0, "respawn": self.respawn}

    def actions(self, seeds, t, n_agents):
        """The row's action stream at step t: int32 [len(seeds)][n_agents][3] (zs_gen_actions' for "discrete")."""
        if self.stream == "discrete":
            return np.array([[A.DISCRETE_TRIPLES[A.discrete_action_id(s, t, a, 7)] for a in range(n_agents)]
                             for s in seeds], dtype=np.int32)
        return np.array([[A.encode_action(A.rich_action(s, t, a)) for a in range(n_agents)] for s in seeds],
                        dtype=np.int32)


ROWS = [Row(G, k, cfg, reg) for (G, k), (cfg, reg) in _ROWS.items()]
SMALL_ROWS = [Row(G, k, cfg, reg, n) for (G, k, n), (cfg, reg) in _SMALL.items()]


def all_instantiations():
    """The 21 (G, kernel) of k_tick_g.hip's seven translation units."""
    return [(G, k) for G in GS for k in KERNELS]


def min_image_args(builder, G, fused):
    """The arguments (step_plan_table.images) of the smallest image the plan tries for G lanes per env: a 32-word
    RNG window, no spawn-candidate copy, no spawn lists, no observation image."""
    c, m = builder.cfg, builder.cfg.map
    E = c.num_agents + c.num_bots + max(c.initial_zombies, c.minimum_zombies)
    cells = m.width * m.height
    ncand = max(m.n_player_spawns or cells, m.n_zombie_spawns or cells)
    return (int(fused), 64 // G, E, (cells + 31) // 32, 32, 0, 0, c.num_agents, ncand, 0)


def census(row, steps=STEPS):
    """The oracle's census (oracle.CENSUS_EXT, summed over the row's envs) of the row's config, seeds, action stream
    and step count at chunk size G, autoresets included."""
    from oracle.oracle import OracleEnv, run_hashes
    if row.stream == "discrete":
        return run_hashes(row.make(1), row.seed0, row.n, steps, 7, chunk_g=row.G)[1]
    tot = {}
    for s in row.seeds():
        o = OracleEnv(row.make(1))
        o.seed(s)
        o.reset()
        o.set_census(row.G)
        need = False
        for t in range(1, steps + 1):
            if need:
                o.reset()
                need = False
            else:
                _, _, d, tr, _ = o.step(row.actions([s], t, o.A)[0])
                need = d or tr
        for k, v in o.census().items():
            tot[k] = max(tot.get(k, 0), v) if k == "max_in_chunk" else tot.get(k, 0) + v
    return tot
