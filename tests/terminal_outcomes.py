"""One case per (way an episode can end, lanes per env): the table of test_terminal_outcomes_plan.py (CPU: the
oracle alone shows every outcome a row claims, the compiled step plan resolves every row to its G and kernel) and
test_terminal_outcomes.py (GPU: every env at every step against the oracle, the state at every terminal step and
after every autoreset).

The group path forms the rule inputs in env_cleanup_group (csrc/zs_tick.hpp) by ballots masked to the env's G
lanes over chunks of G entity slots: zombies present, any player alive, any agent alive, an alive player off the
objectives.  env_step_leader_b turns them into ended / won / truncated and the +-10 end reward (rules_check for
evacuation and for extermination after a same-step respawn) and multi_rewards hands the end reward to agent a
on lane a mod G.  So every outcome runs at every G, with k_step and k_tick alternating over the configs of one G
(tick_waves 5 and 6 alternate with them) and both par_exec = 1 and par_exec = -1 in every case.

Outcomes (outcomes.py): ext_won, ext_lost, ext_min_won (no free spawn cell), ext_min_goes_on (a free one), safe_won,
safe_lost, evac_won, evac_lost, evac_apart, surv_lost, agents_dead_bot_alive (multi and single surface),
done_and_timelimit, single_won / single_lost (ZS_REWARD_SINGLE's end reward); and late_player / late_zombie /
late_off: the decisive thing (the only player alive, the only zombie left, the only alive player off the
objectives) in an entity slot >= G, so that a later chunk of the ballot loop decides.  The teams here hold two to
four players, so the late_* outcomes are claimed at G = 1 and 2 (LATE_GS below); the same rows have more agents than
lanes (A > G: the end reward and `listed` of the agents beyond the first lanes).

Respawn: the one-cell spawn list of one_spawn.txt is placed by the tick (ext_min), or by k_respawn under
zs_launch.defer_respawn = 1 (ext_min_defer); the 68 cells of WIDE_MAP are past step_defer_respawn()'s 64, so
k_respawn is the plan's own choice (ext_wide).  ext_min_won needs every spawn cell occupied, which no stream
reaches with 68 cells.

Env counts, steps: step_instantiations.ENVS and STEPS (two workgroups or more, the last one partial; 24 steps).
Episodes are short (a TimeLimit of 6 or 8 steps, or a crowd that kills the players in a few), so envs end,
autoreset and end again.
"""
import os

import outcomes as O
import step_instantiations as S
from libzombsole_amd import _abi
from libzombsole_amd.maps import Map

MAPS = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "maps")

# 14 x 8: four player spawns and 68 zombie spawns (> 64: respawn by k_respawn)
WIDE_MAP = ("wwwwwwwwwwwwww\n"
            "wppzzzzzzzzzzw\n"
            "wppzzzzzzzzzzw\n"
            "wzzzzzzzzzzzzw\n"
            "wzzzzzzzzzzzzw\n"
            "wzzzzzzzzzzzzw\n"
            "wzzzzzzzzzzzzw\n"
            "wwwwwwwwwwwwww\n")


def _map(name):
    return Map.from_file(os.path.join(MAPS, name + ".txt"))


def _ids(n):
    return [str(i) for i in range(n)]


def _multi(n, rules, bots, map_, agents, z, zmin, ms, weapons="rifle", dlog=False):
    b = _abi.multi_env_config(n, rules, bots, map_, _ids(agents), initial_zombies=z, minimum_zombies=zmin,
                              agent_weapons=weapons, max_episode_steps=ms, observation_surroundings_width=7)
    if dlog:
        b.cfg.flags |= _abi.FLAG_DEATH_LOG
    return b


def _single(n, rules, bots, map_, z, zmin, ms, weapon="rifle"):
    return _abi.single_env_config(n, rules, bots, map_, 0, initial_zombies=z, minimum_zombies=zmin,
                                  observation_scope="surroundings:7", observation_position_encoding="channels",
                                  agent_weapon=weapon, max_episode_steps=ms)


# config -> (builder, action stream, describe()'s respawn, further zs_launch overrides, the outcomes its rows claim;
# a late_* outcome with the lane counts it is claimed at)
CONFIGS = {
    "safe_crowd": (lambda n: _multi(n, "safehouse", [], _map("safe_crowd"), 2, 4, 4, 0),
                   "discrete", "tick", {}, ("safe_won", "safe_lost", ("late_off", (1,)), ("late_player", (1,)))),
    "safe_tiny": (lambda n: _multi(n, "safehouse", [], _map("safe_tiny"), 3, 1, 1, 6),
                  "discrete", "tick", {}, ("safe_won", ("late_off", (1, 2)))),
    "evac_tiny": (lambda n: _multi(n, "evacuation", [], _map("evac_tiny"), 4, 2, 2, 6),
                  "discrete", "tick", {}, ("evac_won", "evac_apart", "done_and_timelimit")),
    "evac_bot": (lambda n: _multi(n, "evacuation", ["terminator"], _map("evac_tiny"), 2, 2, 2, 6),
                 "rich", "tick", {}, ("evac_won", "evac_apart")),
    "evac_crowd": (lambda n: _multi(n, "evacuation", [], _map("evac_crowd"), 4, 9, 9, 0, "knife", dlog=True),
                   "discrete", "tick", {}, ("evac_lost", "evac_apart")),
    "surv_melee": (lambda n: _multi(n, "survival", [], _map("melee"), 4, 14, 14, 0, dlog=True),
                   "discrete", "tick", {}, ("surv_lost", ("late_player", (1, 2)))),
    "multi_troll": (lambda n: _multi(n, "survival", ["troll"], _map("melee"), 1, 14, 14, 0),
                    "discrete", "tick", {}, ("agents_dead_bot_alive",)),
    "single_troll": (lambda n: _single(n, "survival", ["troll"], _map("melee"), 14, 14, 0),
                     "discrete", "tick", {}, ("agents_dead_bot_alive", "single_lost")),
    "single_duel": (lambda n: _single(n, "extermination", [], _map("one_spawn"), 1, 0, 8),
                    "discrete", "tick", {}, ("single_won",)),
    "ext_duel": (lambda n: _multi(n, "extermination", [], _map("one_spawn"), 2, 1, 0, 8, "axe"),
                 "discrete", "tick", {}, ("ext_won", ("late_zombie", (1, 2)))),
    "ext_melee": (lambda n: _multi(n, "extermination", [], _map("melee"), 4, 14, 0, 0, "knife"),
                  "rich", "tick", {}, ("ext_lost",)),
    "ext_min": (lambda n: _multi(n, "extermination", [], _map("one_spawn"), 2, 1, 1, 8, "axe", dlog=True),
                "discrete", "tick", {}, ("ext_min_won", "ext_min_goes_on")),
    "ext_min_defer": (lambda n: _multi(n, "extermination", [], _map("one_spawn"), 2, 1, 1, 8, "axe"),
                      "discrete", "k_respawn", {"defer_respawn": 1}, ("ext_min_won", "ext_min_goes_on")),
    "ext_wide": (lambda n: _multi(n, "extermination", [], Map.from_text(WIDE_MAP, name="wide"), 2, 1, 1, 8, "shotgun"),
                 "discrete", "k_respawn", {}, ("ext_min_goes_on",)),
}

# every outcome the rows of one G must provide between them, and the late_* ones at the lane counts LATE_GS
LATE_GS = (1, 2)
OUTCOMES = ("ext_won", "ext_lost", "ext_min_won", "ext_min_goes_on", "safe_won", "safe_lost", "evac_won", "evac_lost",
            "evac_apart", "surv_lost", "agents_dead_bot_alive", "done_and_timelimit", "single_won", "single_lost")
LATE = ("late_player", "late_zombie", "late_off")
# (G, config) -> why the plan cannot run the config at that G (the step_plan() condition); none: every config's
# image fits 64 KiB at every G (test_terminal_outcomes_plan.py holds the plan to it)
UNREACHABLE = {}
# rows whose first seed is moved so that every claimed outcome shows in three envs or more (the plan test counts)
SEED0 = {(8, 'single_troll'): 27314, (64, 'safe_crowd'): 20607, (64, 'single_troll'): 27642, (64, 'ext_min_defer'): 32614}


class Row(S.Row):
    def __init__(self, G, kernel, config, ci):
        self.G, self.kernel, self.config = G, kernel, config
        self.n = S.ENVS[G]
        self.make, self.stream, self.respawn, extra, claims = CONFIGS[config]
        self.claims = tuple(c for c in claims if isinstance(c, str)) + \
            tuple(c[0] for c in claims if not isinstance(c, str) and G in c[1])
        launch, self.step_kernel, self.tick_waves = S.KERNEL_LAUNCH[kernel]
        self.launch = dict(launch, fobs=-1, **extra)
        self.fused = kernel == "k_step"
        self.id = "G%d-%s-%s@%d" % (G, kernel, config, self.n)
        self.seed0 = SEED0.get((G, config), 20000 + 1000 * ci + 100 * S.GS.index(G))

    def info(self):
        return O.info_for(self.make(1), self.G)


ROWS = [Row(G, S.KERNELS[(ci + gi) % 3], cfg, ci) for gi, G in enumerate(S.GS) for ci, cfg in enumerate(CONFIGS)
        if (G, cfg) not in UNREACHABLE]


def census(row, steps=S.STEPS):
    """The oracle alone over the row's config, seeds, stream and steps: outcome -> the number of envs it occurs
    in, and "late_terminal": the envs that end at an episode's second step or later."""
    from oracle.oracle import OracleEnv
    info, got = row.info(), {}
    for s in row.seeds():
        o = OracleEnv(row.make(1))
        o.seed(s)
        o.reset()
        prev, need, ep, seen = o.state(), False, 0, set()
        for t in range(1, steps + 1):
            if need:
                o.reset()
                need, ep = False, 0
            else:
                _, _, d, tr, _ = o.step(row.actions([s], t, o.A)[0])
                ep += 1
                cur = o.state()
                seen |= O.classify(info, prev, cur, d, tr)
                need = d or tr
                if need and ep > 1:
                    seen.add("late_terminal")
                if need:
                    seen.add("terminal")
            prev = o.state()
        for k in seen:
            got[k] = got.get(k, 0) + 1
    return got
