"""The scripted policies for agent slots in numpy: the second statement of their rules (the first is
csrc/zs_autopilot.hpp).

    decide(state, map, A, policy) -> int32 [A, 3]

A row is an agent's action triple (ACT_*, dx, dy) in zs_step's form, computed from the env's current world under the
agent's policy code:
  NONE        the row is not written (zero in a fresh result, untouched in `out`)
  TERMINATOR  players/terminator.py with the agent's own weapon.  z = the closest present zombie by (d2, rank in the dict
              order): closest() keeps the first minimum it meets walking World.things.  No zombie: (HEAL, 0, 0).
              d2 <= the weapon's range: (ATTACK_CLOSEST, 0, 0).  Else the adjacent cell of minimal d2 to z, the first
              minimum in adjacent_positions order (0,1), (0,-1), (1,0), (-1,0): (HEAL, dx, dy) when a present agent or
              bot stands there, (ATTACK, dx, dy) when any other present thing does (a zombie; an obstacle whatever its
              life), else (MOVE, dx, dy), outside the map too
  SNIPER      players/sniper.py: (ATTACK_CLOSEST, 0, 0)
  TROLL       players/troll.py: (HEAL, 0, 0)
  other codes (IDLE, 0, 0); the kernel also raises OVF_PARAM_RANGE
An agent of nonzero code that is not present gets (IDLE, 0, 0).  Agent.next_step resolves every such triple to the
(action, target) the bot class returns, so stepping with them is stepping the bot in the agent's place.

`state` is an engine.StateView (Engine.get_state) or anything with its fields: `ent` [E][>= 6] rows of (kind, present,
x, y, life, weapon), slots agents [0, A), bots [A, A + P), zombies after them; `order` (the present slots in dict order)
and `n_order`; `obst_present` [O]; `P`.  `map` is an entity_obs.Static.
"""
import numpy as np

from . import actions as ACT
from .entity_obs import Static, weapon_r2  # noqa: F401  (Static: what decide reads of a map)

NONE, TERMINATOR, SNIPER, TROLL = 0, 1, 2, 3
POLICIES = {"none": NONE, "terminator": TERMINATOR, "sniper": SNIPER, "troll": TROLL}
ADJACENT = ((0, 1), (0, -1), (1, 0), (-1, 0))  # adjacent_positions order (utils.py:34-44)

_NAME_BY_KIND = {ACT.ACT_MOVE: "move", ACT.ACT_ATTACK: "attack", ACT.ACT_ATTACK_CLOSEST: "attack_closest",
                 ACT.ACT_HEAL: "heal", ACT.ACT_HEAL_CLOSEST: "heal_closest"}


def policy_code(policy):
    """A policy's code from its name or its code."""
    if isinstance(policy, str):
        if policy not in POLICIES:
            raise ValueError("%r is not a scripted policy: one of %s" % (policy, ", ".join(sorted(POLICIES))))
        return POLICIES[policy]
    return int(policy)


def to_action_dict(triple):
    """The reference's action dict of a triple: what Agent.set_action takes, and what actions.encode_action maps back
    to the triple."""
    kind, dx, dy = (int(v) for v in triple)
    return {"action_type": _NAME_BY_KIND.get(kind), "parameter": [dx, dy]}


def decide(state, map, A, policy, out=None):
    ent = state.ent
    E, P = len(ent), int(state.P)
    A = int(A)
    codes = [policy_code(policy)] * A if isinstance(policy, (str, int, np.integer)) else [int(c) for c in policy]
    res = np.zeros((A, 3), dtype=np.int32) if out is None else out
    rank = {int(s): k for k, s in enumerate(state.order[:int(state.n_order)])}
    at = {(int(ent[s][2]), int(ent[s][3])): s for s in range(E) if int(ent[s][1])}
    zombies = [s for s in range(A + P, E) if int(ent[s][1])]
    for a in range(A):
        code = codes[a]
        if code == NONE:
            continue
        row = (ACT.ACT_IDLE, 0, 0)
        if int(ent[a][1]) and code in (TERMINATOR, SNIPER, TROLL):
            ax, ay = int(ent[a][2]), int(ent[a][3])
            if code == SNIPER:
                row = (ACT.ACT_ATTACK_CLOSEST, 0, 0)
            elif code == TROLL or not zombies:
                row = (ACT.ACT_HEAL, 0, 0)
            else:
                d2, _, z = min(((int(ent[s][2]) - ax) ** 2 + (int(ent[s][3]) - ay) ** 2, rank.get(s, 0xffff), s) for s in zombies)
                if d2 <= weapon_r2(ent[a][5]):
                    row = (ACT.ACT_ATTACK_CLOSEST, 0, 0)
                else:
                    zx, zy = int(ent[z][2]), int(ent[z][3])
                    _, k = min(((zx - ax - dx) ** 2 + (zy - ay - dy) ** 2, k) for k, (dx, dy) in enumerate(ADJACENT))
                    dx, dy = ADJACENT[k]
                    cell = (ax + dx, ay + dy)
                    o = map.obstacle_at.get(cell)
                    kind = ACT.ACT_MOVE
                    if 0 <= cell[0] < map.W and 0 <= cell[1] < map.H:
                        if o is not None and int(state.obst_present[o]):
                            kind = ACT.ACT_ATTACK
                        elif cell in at:
                            kind = ACT.ACT_HEAL if at[cell] < A + P else ACT.ACT_ATTACK
                    row = (kind, dx, dy)
        res[a] = row
    return res
