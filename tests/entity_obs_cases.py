"""Shared by the entity-observation tests: plain state views, the text form tests/entity_obs_host.cpp reads, the GPU
rows (the maps of render_cases.ROWS) with their oracle-side trace and census, and the classes every row must show by
the oracle alone (test_entity_obs_plan.py) before test_entity_obs.py may claim them.
"""
import functools

import numpy as np

import render_cases as RC
from libzombsole_amd import _abi
from libzombsole_amd import entity_obs as EO

KS = ((1, 0), (4, 1), (16, 16))
CENSUS_K = (4, 1)  # the K values the census classes are counted at
CLASSES = ("tie", "truncated", "short", "absent_agent", "in_range", "out_of_range", "ray_obstacle", "ray_edge", "ray_cap",
           "on_objective")
ZOMBIE, PLAYER, AGENT = 5, 6, 7


class View(object):
    """A state as encode reads it: ent rows (kind, present, x, y, life, weapon), obstacle presence, A, P."""

    def __init__(self, A, P, ent, obst_present=()):
        self.A, self.P = A, P
        self.ent = np.array([list(e) + [0] * (6 - len(e)) for e in ent], dtype=np.int64).reshape(-1, 6)
        self.obst_present = np.array(list(obst_present), dtype=np.int64)


def ent(present, x, y, life=100, weapon=13, kind=0):
    return (kind, present, x, y, life, weapon)


def host_text(cases):
    """[(view, static, kz, kp)] as the text entity_obs_host reads."""
    lines = [str(len(cases))]
    for v, st, kz, kp in cases:
        lines.append("%d %d %d %d %d %d %d %d %d" % (st.W, st.H, v.A, v.P, len(v.ent), len(st.obstacles), len(st.objectives), kz, kp))
        lines += ["%d %d %d %d %d" % tuple(int(x) for x in e[1:6]) for e in v.ent]
        lines += ["%d %d %d" % (x, y, int(v.obst_present[i])) for i, (x, y) in enumerate(st.obstacles)]
        lines += ["%d %d" % o for o in st.objectives]
    return "\n".join(lines) + "\n"


def slice_rows(full, kz, kp, kz0=16, kp0=16):
    """The rows at (kz, kp) of rows encoded at (kz0, kp0) >= them: the first kz and kp of the same sorted lists."""
    L0, L = EO.layout(kz0, kp0), EO.layout(kz, kp)
    out = np.zeros(full.shape[:-1] + (L["row_words"],), dtype=np.int16)
    out[..., :8] = full[..., :8]
    out[..., L["zombies"]:L["zombies"] + 4 * kz] = full[..., L0["zombies"]:L0["zombies"] + 4 * kz]
    out[..., L["players"]:L["players"] + 4 * kp] = full[..., L0["players"]:L0["players"] + 4 * kp]
    out[..., L["objective"]:] = full[..., L0["objective"]:]
    return out


# ---------------------------------------------------------------------------
# the GPU rows: render_cases' maps, without its render flag
# ---------------------------------------------------------------------------
def _bridge_a4(n, **over):
    opts = dict(max_episode_steps=0)
    opts.update(over)
    return _abi.multi_env_config(n, "extermination", ["terminator", "sniper"], "bridge", ["0", "1", "2", "3"], initial_zombies=20,
                                 minimum_zombies=12, agent_weapons=["knife", "axe", "gun", "shotgun"], **opts)


def builder(row, n, **over):
    if row == "bridge_a4":  # the multi surface with four agents and two bots
        return _bridge_a4(n, **over)
    return RC.ROWS[row](n, render=False, **over)


ROWS = tuple(sorted(RC.ROWS)) + ("bridge_a4",)
SEED0 = RC.SEED0


def steps_of(row):
    return {"bridge_a4": 24, "crowd9x7": 30}.get(row, RC.steps_of(row))


def oracle_view(b, st):
    """A View of an oracle state.  The oracle has no slots: agents and bots take theirs, zombies are numbered in dict
    order, which is enough to count the census classes (no class depends on which of two tied zombies comes first)."""
    A, P = b.num_agents, b.num_bots
    E = A + P + max(b.cfg.initial_zombies, b.cfg.minimum_zombies)
    rows = [[0] * 6 for _ in range(E)]
    z = A + P
    for kind, x, y, life, weapon, extra in st["dyn"]:
        if kind == AGENT:
            s = extra
        elif kind == PLAYER:
            s = A + extra
        else:
            s, z = z, z + 1
        rows[s] = [kind, 1, x, y, life, weapon]
    present = np.ones(len(b.map.obstacles), dtype=np.int64)
    for i, _life, pr in st["obst"]:
        present[i] = pr
    return View(A, P, rows, present)


def classes_of(view, static, kz=CENSUS_K[0], kp=CENSUS_K[1]):
    """The census classes the env's state shows at (kz, kp)."""
    c = set()
    A, np_ = view.A, view.A + view.P
    zs = [s for s in range(np_, len(view.ent)) if view.ent[s][1]]
    rows = EO.encode(view, static, kz, kp)
    L = EO.layout(kz, kp)
    for a in range(A):
        if not view.ent[a][1]:
            c.add("absent_agent")
            continue
        ax, ay = int(view.ent[a][2]), int(view.ent[a][3])
        d = sorted((int(view.ent[s][2]) - ax) ** 2 + (int(view.ent[s][3]) - ay) ** 2 for s in zs)
        if any(d[i] == d[i + 1] for i in range(min(kz, len(d) - 1))):
            c.add("tie")  # two keys that differ in the slot alone, at a rank the row shows (or at its cut)
        if len(zs) > kz:
            c.add("truncated")
        if len(zs) < kz:
            c.add("short")
        for i in range(min(kz, len(zs))):
            c.add("in_range" if rows[a][L["zombies"] + 4 * i + 3] & EO.IN_RANGE else "out_of_range")
        if rows[a][L["objective"] + 2] & EO.ON_OBJECTIVE:
            c.add("on_objective")
        for k, (dx, dy) in enumerate(EO.RAY_DIRS):
            n = int(rows[a][L["rays"] + k])
            cx, cy = ax + (n + 1) * dx, ay + (n + 1) * dy
            if n == EO.RAY_CAP:
                c.add("ray_cap")
            elif not (0 <= cx < static.W and 0 <= cy < static.H):
                c.add("ray_edge")
            else:
                c.add("ray_obstacle")
    return c


@functools.lru_cache(maxsize=None)
def oracle_trace(row, n):
    """(states, census): states[t][k] the oracle's state of env k after t steps (t = 0: the reset), with the autoreset of
    the step after an env ended; census[k] the classes env k showed.  Actions: the device policy's."""
    from libzombsole_amd import actions as A
    from oracle.oracle import OracleEnv
    b = builder(row, 1)
    static = EO.Static.of_map(b.map)
    nA = b.num_agents
    envs, need, census = [], [False] * n, [set() for _ in range(n)]
    for k in range(n):
        o = OracleEnv(builder(row, 1))
        o.seed(SEED0 + k)
        for i, life in RC.POKES.get(row, []):
            if i < len(b.map.obstacles):
                o.poke_obstacle(i, life)
        o.reset()
        envs.append(o)

    def look(k):
        st = envs[k].state()
        census[k] |= classes_of(oracle_view(b, st), static)
        return st

    states = [[look(k) for k in range(n)]]
    for t in range(1, steps_of(row) + 1):
        for k, o in enumerate(envs):
            if need[k]:
                o.reset()
                need[k] = False
                continue
            acts = np.stack([A.DISCRETE_TRIPLES[int(A.discrete_action_id(SEED0 + k, t, a, 7))] for a in range(nA)])
            _obs, _r, d, tr, _l = o.step(acts)
            need[k] = d or tr
        states.append([look(k) for k in range(n)])
    return states, census


def claimed(row, n=13):
    """The classes a row may claim: those at least three of its envs show, by the oracle alone."""
    _states, census = oracle_trace(row, n)
    return {c for c in CLASSES if sum(c in s for s in census) >= 3}


# The classes every row must show in three envs or more of its first 13 (test_entity_obs_plan.py holds the oracle's
# census to this table); together the rows cover every class.
REQUIRED = {
    "bridge64": {"in_range", "out_of_range", "ray_cap", "ray_obstacle", "tie", "truncated"},
    "crowd9x7": {"absent_agent", "in_range", "on_objective", "ray_edge", "ray_obstacle", "tie", "truncated"},
    "field9x7": {"absent_agent", "in_range", "on_objective", "ray_edge", "ray_obstacle", "tie", "truncated"},
    "fort_e132": {"in_range", "out_of_range", "ray_cap", "ray_obstacle", "tie", "truncated"},
    "safe8x5": {"absent_agent", "in_range", "on_objective", "ray_obstacle", "tie"},
    "strip1x70": {"in_range", "on_objective", "out_of_range", "ray_cap", "ray_edge", "truncated"},
    "strip70x1": {"in_range", "on_objective", "out_of_range", "ray_cap", "ray_edge", "truncated"},
    "wall5x4": {"in_range", "ray_obstacle", "short"},
    "bridge_a4": {"in_range", "out_of_range", "ray_cap", "ray_edge", "ray_obstacle", "tie", "truncated"},
}
