"""The action-mask rules (include/zombsole_mi355x.h, zs_action_mask) restated on the host over a canonical state
record (golden_driver.canonical_state / StateView.canonical): `dyn` the things of World.things that are no
obstacle, in dict order, [kind, x, y, life, weapon, extra]; `obst` the obstacles that left their fresh state,
[index, life, present].  test_mask_model.py holds this to the reference's own masks (tests/golden/masks_*.json.gz);
the GPU tests hold the kernel to it on states no fixture covers."""
from libzombsole_amd.maps import load_map

ZOMBIE, PLAYER, AGENT = 5, 6, 7
MOVES = ((0, 1), (-1, 0), (0, -1), (1, 0))  # game_actions[0..3] (gym_env.py:328-351)
# weapons.py:18-25 max_range as the largest integer d2 inside it: 1.5 -> 2, 3 -> 9, 6 -> 36, 10 -> 100
RANGE2 = {10: 2, 11: 2, 12: 36, 13: 100, 14: 9}
HEAL2 = 9  # HEALING_RANGE = 3 (core.py:8)


class MapInfo(object):
    def __init__(self, map_name):
        m = load_map(map_name)
        self.W, self.H = m.size
        self.obstacles = [(o[0], o[1]) for o in m.obstacles]
        self.kinds = [o[2] for o in m.obstacles]
        self.objectives = {tuple(p) for p in m.objectives}
        self.index = {c: i for i, c in enumerate(self.obstacles)}
        self.max_life = [10 if k == 1 else 200 for k in self.kinds]  # Box / Wall MAX_LIFE (things.py)


def obstacle_cells(state, mp):
    """cell -> life of the obstacles in World.things; set of the cells whose obstacle was removed."""
    life = {i: (10 if k == 1 else 200) for i, k in enumerate(mp.kinds)}
    gone = set()
    for i, lf, present in state["obst"]:
        life[i] = lf
        if not present:
            gone.add(i)
    return ({mp.obstacles[i]: lf for i, lf in life.items() if i not in gone}, {mp.obstacles[i] for i in gone})


def d2(a, b):
    return (a[0] - b[0]) ** 2 + (a[1] - b[1]) ** 2


def masks(state, mp, n_agents, n_discrete, heal_r2=HEAL2, dead_obstacles_block=True, others_exclude_self=True):
    """[n_agents][8] of 0/1.  The keyword switches are test_mask_model.py's mutations: each one must make named
    fixture cases fail."""
    changed = {i: (lf, present) for i, lf, present in state["obst"]}
    dyn = state["dyn"]
    things = {(t[1], t[2]) for t in dyn}
    zombies = [(t[1], t[2]) for t in dyn if t[0] == ZOMBIE]

    def free(q):
        if not (0 <= q[0] < mp.W and 0 <= q[1] < mp.H) or q in things:
            return False
        i = mp.index.get(q)
        if i is None:
            return True
        lf, present = changed.get(i, (1, 1))
        return not present or (lf <= 0 and not dead_obstacles_block)

    out = []
    for a in range(n_agents):
        me = [t for t in dyn if t[0] == AGENT and t[5] == a]
        row = [0] * 8
        if me:
            p = (me[0][1], me[0][2])
            for k, (dx, dy) in enumerate(MOVES):
                row[k] = int(free((p[0] + dx, p[1] + dy)))
            row[4] = int(bool(zombies) and min(d2(p, z) for z in zombies) <= RANGE2[me[0][4]])
            row[5] = 1
            if n_discrete > 6:
                others = [(t[1], t[2]) for t in dyn if t[0] in (PLAYER, AGENT) and
                          not (others_exclude_self and t is me[0])]
                row[6] = int(not others or min(d2(p, o) for o in others) <= heal_r2)
        out.append(row)
    return out


def state_of(view, mp):
    """The `dyn` and `obst` of an engine StateView (engine.get_state), without the per-obstacle Python loop of
    StateView.canonical."""
    import numpy as np
    dyn = [[int(v) for v in view.ent[int(s)][[0, 2, 3, 4, 5, 6]]] for s in view.order[:view.n_order]]
    ch = np.nonzero((view.obst_life != mp.max_life) | (view.obst_present == 0))[0]
    return {"dyn": dyn, "obst": [[int(i), int(view.obst_life[i]), int(view.obst_present[i])] for i in ch]}
