"""The entity observation in numpy: the second statement of its rules (the first is csrc/zs_entity_obs.hpp).

    encode(state_view, static, kz, kp) -> int16 [A, 16 + 4 (kz + kp)]

A row holds, in int16 words:
  self       8  present (1), x, y, life, weapon code, weapon_r2, zombies present in the env, other agents and bots present
  zombies    kz x (dx, dy, life, flags): the present zombie slots in ascending order of (d2, slot), where d2 = dx^2 + dy^2
                and dx, dy are the zombie's cell minus the agent's.  flags: 1 valid, 2 d2 <= weapon_r2 of the agent's
                weapon, 4 d2 == 1.  Rows past the present zombies are zero
  players    kp x (dx, dy, life, flags): the present agent and bot slots other than the agent itself, same order.
                flags: 1 valid, 2 d2 <= 9 (HEALING_RANGE), 4 the slot is an agent and not a bot, weapon code << 8
  objective  4  (dx, dy, flags, n_objectives) of the nearest objective cell by (d2, map-file index).  flags: 1 valid,
                2 the agent stands on an objective
  rays       4  towards (0,1), (-1,0), (0,-1), (1,0): the consecutive cells, starting next to the agent, that are
                inside the map and hold no present obstacle, whatever the obstacle's life; at most RAY_CAP.  Entities
                do not stop a ray
Lives and counts saturate to the int16 range.  An agent that is not present has an all-zero row.

`state_view` is an engine.StateView (Engine.get_state) or anything with its fields: `ent` [E][>= 6] rows of (kind,
present, x, y, life, weapon), slots agents [0, A), bots [A, A + P), zombies after them; `obst_present` [O]; `A`; `P`.
`static` is a Static: the map's size, obstacle cells and objective cells in map-file order.

A learner reads a bound tensor with the offsets of layout(kz, kp); the flag constants are below.
"""
import numpy as np

RAY_CAP = 16
HEAL_R2 = 9  # HEALING_RANGE = 3
VALID, IN_RANGE, ADJACENT, IS_AGENT, ON_OBJECTIVE = 1, 2, 4, 4, 2
RAY_DIRS = ((0, 1), (-1, 0), (0, -1), (1, 0))
# a weapon's range as the largest integer d2 inside it: knife and axe 1.5, gun 6, rifle 10, shotgun 3
WEAPON_R2 = {10: 2, 11: 2, 12: 36, 13: 100, 14: 9}


def weapon_r2(code):
    return WEAPON_R2.get(int(code), 2)


def layout(kz, kp):
    """Word offsets of a row's blocks."""
    if not (1 <= kz <= 16 and 0 <= kp <= 16):
        raise ValueError("kz must be in 1..16 and kp in 0..16")
    return {"row_words": 16 + 4 * (kz + kp), "self": 0, "zombies": 8, "players": 8 + 4 * kz,
            "objective": 8 + 4 * (kz + kp), "rays": 12 + 4 * (kz + kp)}


class Static(object):
    """What encode reads of a map: its size, the obstacles' cells (map-file order, the index of `obst_present`) and the
    objective cells (map-file order)."""

    def __init__(self, W, H, obstacles=(), objectives=()):
        self.W, self.H = int(W), int(H)
        self.obstacles = [(int(o[0]), int(o[1])) for o in obstacles]
        self.objectives = [(int(o[0]), int(o[1])) for o in objectives]
        self.obstacle_at = {c: i for i, c in enumerate(self.obstacles)}

    @classmethod
    def of_map(cls, m):
        """From a maps.Map (or a map name / path load_map takes)."""
        from .maps import load_map
        m = load_map(m)
        return cls(m.size[0], m.size[1], m.obstacles, m.objectives)


def _sat(v):
    return max(-32768, min(32767, int(v)))


def _w16(v):
    """The int16 word holding the 16 low bits of v."""
    v = int(v) & 0xffff
    return v - 0x10000 if v >= 0x8000 else v


def _nearest(slots, ent, ax, ay, k):
    """The first k of `slots` that are present, by (d2, slot): [(dx, dy, d2, slot)]."""
    rows = []
    for s in slots:
        if int(ent[s][1]):
            dx, dy = int(ent[s][2]) - ax, int(ent[s][3]) - ay
            rows.append((dx * dx + dy * dy, s, dx, dy))
    rows.sort()
    return [(dx, dy, d2, s) for d2, s, dx, dy in rows[:k]]


def ray(static, obst_present, x, y, dx, dy):
    n = 0
    while n < RAY_CAP:
        cx, cy = x + (n + 1) * dx, y + (n + 1) * dy
        if not (0 <= cx < static.W and 0 <= cy < static.H):
            break
        o = static.obstacle_at.get((cx, cy))
        if o is not None and int(obst_present[o]):
            break
        n += 1
    return n


def encode(state_view, static, kz, kp):
    L = layout(kz, kp)
    ent, A, P = state_view.ent, int(state_view.A), int(state_view.P)
    E = len(ent)
    out = np.zeros((A, L["row_words"]), dtype=np.int16)
    players, zombies = range(0, A + P), range(A + P, E)
    n_zombies = sum(1 for s in zombies if int(ent[s][1]))
    n_players = sum(1 for s in players if int(ent[s][1]))
    for a in range(A):
        if not int(ent[a][1]):
            continue
        ax, ay, life, weapon = (int(v) for v in ent[a][2:6])
        r2 = weapon_r2(weapon)
        row = [0] * L["row_words"]
        row[0:8] = [1, ax, ay, _sat(life), weapon, r2, _sat(n_zombies), _sat(n_players - 1)]
        for i, (dx, dy, d2, s) in enumerate(_nearest(zombies, ent, ax, ay, kz)):
            flags = VALID | (IN_RANGE if d2 <= r2 else 0) | (ADJACENT if d2 == 1 else 0)
            row[L["zombies"] + 4 * i:L["zombies"] + 4 * i + 4] = [dx, dy, _sat(ent[s][4]), flags]
        for i, (dx, dy, d2, s) in enumerate(_nearest([s for s in players if s != a], ent, ax, ay, kp)):
            flags = VALID | (IN_RANGE if d2 <= HEAL_R2 else 0) | (IS_AGENT if s < A else 0) | ((int(ent[s][5]) & 0xff) << 8)
            row[L["players"] + 4 * i:L["players"] + 4 * i + 4] = [dx, dy, _sat(ent[s][4]), flags]
        if static.objectives:
            d2, i = min(((ox - ax) ** 2 + (oy - ay) ** 2, i) for i, (ox, oy) in enumerate(static.objectives))
            ox, oy = static.objectives[i]
            row[L["objective"]:L["objective"] + 4] = [ox - ax, oy - ay, VALID | (ON_OBJECTIVE if d2 == 0 else 0),
                                                      _sat(len(static.objectives))]
        row[L["rays"]:L["rays"] + 4] = [ray(static, state_view.obst_present, ax, ay, dx, dy) for dx, dy in RAY_DIRS]
        out[a] = [_w16(v) for v in row]
    return out
