"""Directed workloads for the decision half of World.step: Zombie.next_step, the scripted bots, Agent.next_step's
closest() calls, and the range tests of World.thing_attack / thing_heal.  One row per shape that forces a branch the
random workloads reach only by chance (DESIGN.md has the measured table): the oracle's decision census
(oracle.CENSUS_DECISIONS, counted from the reference's own statements) names the branches, every row names the
counters it claims, test_decision_plan.py holds the claims to the oracle's run on the CPU, test_decisions.py runs
every row on the GPU against the oracle, and the rows with `fixture` are recorded from the reference itself
(tests/golden/dec_*.json.gz, through make_golden.py) and replayed by the three golden tests.

The maps (tests/golden/maps/dec_*.txt) are a few dozen cells with spawn lists of one to five cells, so a handful
of seeds enumerates the placements:

  dec_corr_h    a one-cell corridor of four zombie spawns, a player spawn at either end, a wall above (neighbour 1
                of adjacent_positions) and boxes below (neighbour 0): the zombie next to the player attacks, the
                next one is at d^2 = 4, every other one is blocked with a zombie on the neighbour towards the player
                (neighbours 2 and 3) and its two obstacle neighbours tied; the boxes break and open the way
  dec_corr_v    the same upright: wall left (neighbour 3), boxes right (neighbour 2), zombies on neighbours 0 and 1
  dec_cross     five zombie spawns in a plus, player spawns in the corners: the centre zombie stands among four
                zombies and no obstacle (idle), the arm's zombie next to a corner is at d^2 = 2, the next at d^2 = 4
  dec_pen       a zombie spawn and a player spawn walled into the top corners: both in-map neighbours are taken, so
                the zombie's (the hamster's, the randoman's) only free cells are off the map
  dec_square    a zombie spawn with four player spawns at d^2 = 4 round it; dec_square_r the reverse, for the
                players' closest() calls.  The discrete stream's moves re-insert the movers at the end of the
                dict order, so ties are decided against creation order
  dec_edge      four player spawns, each with walls at (1,1) (2,0) | (3,0) (3,1) | (6,0) (6,1) | (10,0) (10,1) from
                it: a knife's or axe's, a shotgun's or a heal's, a gun's and a rifle's range and the next d^2 a
                grid has; a fixed script aims at those cells in turn
  dec_wander    survival without autoreset, stepped on after the only player has died: three zombies round the player
                spawn in a walled room whose cells have one to four free neighbours, a fourth walled in
  dec_term      terminator and sniper: a box and an agent in the way, a zombie spawn three cells off on both axes
                (two adjacent cells tie for the best), zombies that are not kept up, so that the bots end
                without a target
  dec_ham       a player spawn walled in on four sides in the map (a stuck hamster) and one in the open
"""
import numpy as np

import golden_util
from libzombsole_amd import actions as A

STEPS = 24
ENVS = {1: 37, 8: 37, 64: 13}   # requested lanes per env -> envs (test_decisions.py)
N_PLAN = 13                     # the claims hold for the first 13 seeds of a row already (test_decision_plan.py)
KEEP_PAST_END = 12              # the wander row: steps taken after the step that ends the episode


def _atk(dx, dy):
    return {"action_type": "attack", "parameter": [dx, dy]}


def _heal(dx, dy):
    return {"action_type": "heal", "parameter": [dx, dy]}


HEAL_SELF = _heal(0, 0)
# dec_edge: the walls at and just past every range, then the two cells a heal reaches and misses
EDGE_SCRIPT = [_atk(1, 1), _atk(2, 0), _atk(3, 0), _atk(3, 1), _atk(6, 0), _atk(6, 1), _atk(10, 0), _atk(10, 1),
               _heal(3, 0), _heal(3, 1)]
# dec_cross: a corner's knife at the arm's zombie (d^2 = 2) and at the arm's end (d^2 = 4), whichever corner it is
CROSS_SCRIPT = [_atk(1, 1), _atk(2, 0), _atk(-1, 1), _atk(-2, 0), _atk(1, -1), _atk(-1, -1), HEAL_SELF]


class Row(object):
    """surface, kwargs: the reference's constructor (golden_util.builder_for reads them); stream: "discrete",
    "rich" or "script" (script[agent][(step - 1) % len], dict actions); max_steps: the TimeLimit; keep: no autoreset,
    the env is stepped on after it ended; claims: the census counters (>= 1 each over N_PLAN envs and STEPS steps);
    fixture: (seeds, calls, the counters the recorded run itself shows) or None."""

    def __init__(self, rid, surface, stream, kwargs, claims, script=None, max_steps=8, keep=False, fixture=None,
                 seed0=0, events=False):
        self.id, self.surface, self.stream, self.kwargs = rid, surface, stream, dict(kwargs)
        self.claims, self.script, self.max_steps, self.keep, self.fixture = tuple(claims), script, max_steps, keep, fixture
        self.seed0, self.events = seed0, events
        self.n_agents = 1 if surface == "single" else len(kwargs["agent_ids"])

    @property
    def extras(self):
        e = {}
        if self.script:
            e["script"] = [self.script[a % len(self.script)] for a in range(self.n_agents)]
        if self.keep:
            e["keep_stepping"] = True
        if self.events:  # the fixture also records World.events: the messages of every executed action
            e["events"] = True
        return e

    def fx(self):
        """What golden_util.builder_for takes."""
        return {"name": "dec_" + self.id, "surface": self.surface, "stream": self.stream, "kwargs": self.kwargs,
                "max_steps": self.max_steps, "extras": self.extras}

    def make(self, n):
        return golden_util.builder_for(self.fx(), num_envs=n)

    def builder(self, n, G=0, kernel="k_tick", par_exec=1):
        b = self.make(n)
        b.cfg.lanes_per_env = G
        return b.set_launch({"fobs": -1, "fused": 1 if kernel == "k_step" else -1, "par_exec": par_exec})

    def seeds(self, n):
        return [self.seed0 + i for i in range(n)]

    def action(self, seed, t, a):
        """Agent a's action at step t as the engine's triple."""
        if self.stream == "discrete":
            return A.DISCRETE_TRIPLES[A.discrete_action_id(seed, t, a, 6 if self.surface == "single" else 7)]
        if self.stream == "script":
            s = self.extras["script"][a]
            return A.encode_action(s[(t - 1) % len(s)])
        return A.encode_action(A.rich_action(seed, t, a))

    def actions(self, seeds, t, n_agents):
        return np.array([[self.action(s, t, a) for a in range(n_agents)] for s in seeds], dtype=np.int32)

    def golden_config(self):
        """The make_golden.CONFIGS entry of a fixture row."""
        seeds, calls, _ = self.fixture
        return ("dec_" + self.id, self.surface, self.stream, self.kwargs, list(seeds), calls, 1, self.max_steps,
                self.extras)


def _multi(map_name, agents, bots, zombies, minimum=0, rules="survival", weapons="rifle", width=5):
    return dict(rules_name=rules, player_names=list(bots), map_name=map_name,
                agent_ids=[str(i) for i in range(agents)], initial_zombies=zombies, minimum_zombies=minimum,
                agent_weapons=weapons, observation_surroundings_width=width)


def _single(map_name, bots, zombies, minimum=0, rules="survival", weapon="rifle", scope="world"):
    return dict(rules_name=rules, player_names=list(bots), map_name=map_name, agent_id=0, initial_zombies=zombies,
                minimum_zombies=minimum, observation_scope=scope, observation_position_encoding="channels",
                agent_weapon=weapon)


_EDGES_4 = tuple("hit_edge_%s_%s" % (s, w) for s in ("in", "out") for w in ("axe", "shotgun", "gun", "rifle", "heal"))

ROWS = [
    # the corridors: the agent heals itself, the zombies queue
    Row("corr_h", "multi", "script", _multi("dec_corr_h", 1, [], 4, weapons="knife"),
        ("z_attack", "z_range_edge_out", "z_blocked_obst_later", "z_blocked_skip_dir2", "z_blocked_skip_dir3",
         "z_blocked_tie", "z_move", "z_move_offmap"), script=[[HEAL_SELF]],
        fixture=([0, 1, 2, 3], 30, ("z_blocked_obst_later", "z_blocked_skip_dir2", "z_blocked_skip_dir3",
                                    "z_blocked_tie", "z_move_offmap"))),
    Row("corr_v", "multi", "script", _multi("dec_corr_v", 1, [], 4, weapons="knife"),
        ("z_attack", "z_range_edge_out", "z_blocked_obst_later", "z_blocked_skip_dir0", "z_blocked_skip_dir1",
         "z_blocked_tie", "z_move"), script=[[HEAL_SELF]],
        fixture=([0, 1, 2, 3], 30, ("z_blocked_obst_later", "z_blocked_skip_dir0", "z_blocked_skip_dir1",
                                    "z_blocked_tie"))),
    # both ends taken: the middle zombies have a zombie on either side
    Row("corr_h2", "multi", "script", _multi("dec_corr_h", 2, [], 4, weapons="axe"),
        ("z_attack", "z_blocked_obst_later", "z_blocked_tie"), script=[[HEAL_SELF]]),
    Row("corr_v2", "multi", "discrete", _multi("dec_corr_v", 2, [], 4, weapons="axe"),
        ("z_attack", "z_blocked_obst_later", "z_blocked_tie")),
    Row("cross", "multi", "script", _multi("dec_cross", 1, [], 5, weapons="knife"),
        ("z_blocked_idle", "z_attack_diag", "z_range_edge_out", "z_move_tie", "z_move_offmap", "hit_edge_in_claws",
         "hit_edge_in_knife", "hit_edge_out_knife"), script=[CROSS_SCRIPT],
        fixture=([0, 1, 2, 3], 30, ("z_blocked_idle", "z_attack_diag", "z_move_tie", "hit_edge_in_claws",
                                    "hit_edge_in_knife", "hit_edge_out_knife"))),
    Row("cross_move", "multi", "discrete", _multi("dec_cross", 2, [], 5, weapons="knife"),
        ("z_blocked_idle", "z_attack_diag", "z_move_tie", "hit_edge_in_claws", "hit_edge_out_claws", "c_tie_zombie")),
    # alone: heal_closest finds no other player
    Row("cross_solo", "multi", "discrete", _multi("dec_cross", 1, [], 5, weapons="axe"),
        ("hc_self_only", "c_none_agent_heal", "z_blocked_idle", "z_attack_diag")),
    Row("pen", "multi", "discrete", _multi("dec_pen", 1, ["hamster", "randoman"], 2, minimum=2, weapons="gun"),
        ("z_move_offmap", "h_move_offmap", "r_move_offmap", "h_move_n2", "r_move") +
        tuple("r_%s_%s" % (k, t) for k in ("attack", "heal") for t in ("obstacle", "self", "player", "zombie")),
        fixture=([0, 1, 2, 3, 4, 5], 40, ("z_move_offmap", "h_move_offmap", "r_move_offmap"))),
    Row("square", "multi", "discrete", _multi("dec_square", 4, [], 1, minimum=1, weapons="shotgun"),
        ("c_tie_zombie", "c_tie_order_zombie", "c_tie_agent_heal", "c_tie_order_agent_heal", "hit_edge_out_claws"),
        fixture=([0, 1, 2, 3], 40, ("c_tie_zombie", "c_tie_order_zombie", "c_tie_agent_heal",
                                    "c_tie_order_agent_heal"))),
    Row("square_r", "multi", "discrete", _multi("dec_square_r", 1, ["terminator", "sniper"], 4, minimum=4,
                                                 weapons="knife"),
        ("c_tie_agent_attack", "c_tie_order_agent_attack", "c_tie_terminator", "c_tie_order_terminator",
         "c_tie_sniper", "c_tie_order_sniper"),
        fixture=([0, 1, 2, 3], 40, ("c_tie_agent_attack", "c_tie_order_agent_attack", "c_tie_terminator",
                                    "c_tie_order_terminator", "c_tie_sniper", "c_tie_order_sniper"))),
    Row("edge", "multi", "script", _multi("dec_edge", 4, [], 0, weapons=["axe", "shotgun", "gun", "rifle"]),
        _EDGES_4, script=[EDGE_SCRIPT], max_steps=12, events=True,
        fixture=([0], 24, _EDGES_4)),
    Row("edge_knife", "multi", "script", _multi("dec_edge", 2, [], 0, weapons=["knife", "axe"]),
        ("hit_edge_in_knife", "hit_edge_out_knife", "hit_edge_in_axe", "hit_edge_out_axe"), script=[EDGE_SCRIPT],
        max_steps=12),
    Row("wander", "single", "script", _single("dec_wander", [], 4, weapon="knife"),
        ("z_wander_n1", "z_wander_n2", "z_wander_n3", "z_wander_n4", "z_wander_stuck", "c_none_zombie",
         "z_blocked_obst_first"), script=[[_atk(-1, 0)]], max_steps=0, keep=True,
        fixture=([0, 1, 2, 3], 40, ("z_wander_n1", "z_wander_n2", "z_wander_n3", "z_wander_n4", "z_wander_stuck",
                                    "z_blocked_obst_first"))),
    # one row per bot type
    Row("terminator", "multi", "discrete", _multi("dec_term", 1, ["terminator"], 3, weapons="knife"),
        ("t_heal_self", "t_attack", "t_move", "t_attack_obstacle", "t_heal_blocker", "t_range_edge_in",
         "t_range_edge_out", "t_move_tie", "c_none_terminator"), max_steps=20),
    Row("sniper", "multi", "discrete", _multi("dec_term", 1, ["sniper"], 3, weapons="rifle"),
        ("s_attack", "s_idle", "c_none_sniper", "c_none_agent_attack"), max_steps=20),
    Row("hamster", "multi", "discrete", _multi("dec_ham", 1, ["hamster"], 1, minimum=1, weapons="gun"),
        ("h_move_n1", "h_move_n2", "h_move_n3", "h_move_n4", "h_move_offmap", "h_stuck")),
    Row("randoman", "multi", "rich", _multi("dec_ham", 1, ["randoman"], 1, minimum=1, weapons="shotgun"),
        ("r_move", "r_move_offmap") +
        tuple("r_%s_%s" % (k, t) for k in ("attack", "heal") for t in ("obstacle", "self", "player", "zombie"))),
]
for _i, _r in enumerate(ROWS):
    _r.seed0 = 71000 + 100 * _i
BY_ID = {r.id: r for r in ROWS}
FIXTURES = [r for r in ROWS if r.fixture]
GRAPHED = ("corr_h", "square_r")  # also through step_graph (test_decisions.py)

# Classes the reference's code cannot reach, with the argument from its lines.
UNREACHABLE = {
    # terminator.py:15-16: best_move is taken only when distance(self, target) > 3, target being the closest zombie.
    # A zombie on best_move, a cell next to the terminator, would be at distance 1: closer than the closest one.
    "t_best_zombie": "a zombie on an adjacent cell is within range, so the terminator attacks and never chases",
    # terminator.py:16: closest(target, adjacent_positions(self)).  The target is on the map and more than 3 away, so
    # on some axis it is 2 or more cells off, and the step along that axis is nearer to it than the terminator's own
    # cell; an off-map neighbour lies across a border the target is inside of, so it is farther from the target than
    # the terminator's own cell.  The nearest neighbour is therefore never off the map.
    "t_best_offmap": "the adjacent cell nearest an on-map target is nearer than the own cell; an off-map one is farther",
}


def golden_configs():
    return [r.golden_config() for r in FIXTURES]


def oracle_census(row, seeds, steps=STEPS, calls=None):
    """The oracle alone over the row's config, stream and seeds, summed.  steps: run_engines' protocol (a reset takes
    a step's place); calls: the fixtures' (call 0 is the reset), the same thing one off."""
    from oracle.oracle import OracleEnv
    tot = {}
    last = steps if calls is None else calls - 1
    for s in seeds:
        o = OracleEnv(row.make(1))
        o.seed(s)
        o.reset()
        need, past = False, 0
        for t in range(1, last + 1):
            if need and not row.keep:
                o.reset()
                need = False
                continue
            _, _, d, tr, _ = o.step(row.actions([s], t, o.A)[0])
            need = d or tr
            past += need
        if row.keep:
            assert past > KEEP_PAST_END, (row.id, s, past)
        for k, v in o.census().items():
            tot[k] = max(tot.get(k, 0), v) if k == "max_in_chunk" else tot.get(k, 0) + v
    return tot
